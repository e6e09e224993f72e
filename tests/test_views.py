"""A batch of camera views in one pipeline run (pt_render_views, pt_render_views_host, pt_views_floats, pt_views_work_bytes,
ptrender --views / --cam-pos / --cam-rot / --fov): the C-ABI surface, the sizes and the argument checks on the CPU; on the GPU
equality of bits, view by view, with the single-camera render (view order, first passes, shading schedules and hand-over thresholds,
the per-pass means, side effects, the CLI) and with the CPU oracle's render of each camera as the check that is not the code under
test.  Bits everywhere, no tolerances."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ptamd
from scenes_util import test_spheres as make_test_spheres
from stats_ref import fold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTRENDER = os.path.join(ROOT, "pathtrace-on-cuda_amd", "ptrender")
NEW_SYMBOLS = ("pt_views_floats", "pt_views_work_bytes", "pt_render_views", "pt_render_views_host")
# (pos, rot, fovy): the reference application's camera, a dolly + yaw, a sideways and upward move with a longer lens
CAMERAS = (((0.0, 20.0, 60.0), (0.0, 90.0, 0.0), 45.0), ((0.0, 20.0, 53.0), (0.0, 93.5, 0.0), 45.0), ((14.0, 23.5, 60.0), (0.0, 97.0, 0.0), 35.0))
FRAMES = ((64, 48), (100, 52))      # whole tiles, and ragged on both edges
PASSES, SPP = 3, 4
SEED_LIMIT = 0x7FFFFFFF             # W * H * (first_pass + passes) must fit an int (srcs/pathtracer.cu:71)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cams(W, H, which=(0, 1, 2)):
    return [ptamd.make_camera(W, H, pos=CAMERAS[i][0], rot_deg=CAMERAS[i][1], fovy_deg=CAMERAS[i][2]) for i in which]


def params(**kw):
    return ptamd.default_params(**{**dict(passes=PASSES, spp_per_pass=SPP), **kw})


def n_tiles_of(W, H):
    return ((W + 7) // 8) * ((H + 7) // 8)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: C-ABI surface, sizes, argument checks, the CLI's options (no device is touched)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound():
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in NEW_SYMBOLS:
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    for name in ("render_views", "render_views_device"):
        assert callable(getattr(ptamd.Scene, name))
    for name in ("views_floats", "views_work_bytes"):
        assert callable(getattr(ptamd, name))


def test_sizes_are_those_of_a_frame_with_as_many_tiles():
    l = ptamd.lib()
    one = ptamd.default_params(rank=0, world=1)
    for W, H in FRAMES + ((240, 136), (1920, 1080)):
        cam = ptamd.make_camera(W, H)
        tx, ty = (W + 7) // 8, (H + 7) // 8
        for V in (1, 3, 16):
            assert ptamd.views_floats(cam, V) == V * ptamd.tiles_floats(cam, one), (W, H, V)
            for prm in (ptamd.default_params(passes=8), ptamd.default_params(passes=2, first_pass=3)):
                cam2 = ptamd.make_camera(8 * tx, 8 * ty * V)
                prm2 = ptamd.PtParams.from_buffer_copy(prm)
                prm2.first_pass, prm2.rank, prm2.world = 0, 0, 1
                assert ptamd.views_work_bytes(cam, prm, V) == ptamd.work_bytes(cam2, prm2), (W, H, V)
    cam, prm = ptamd.make_camera(64, 48), params()
    bc, bp = C.byref(cam), C.byref(prm)
    assert ptamd.views_work_bytes(cam, prm, 1) == ptamd.work_bytes(cam, prm)
    for a in ((None, 3), (bc, 0), (bc, -1), (C.byref(ptamd.make_camera(1, 8)), 3)):
        assert l.pt_views_floats(*a) == -1, a
    for a in ((None, bp, 3), (bc, None, 3), (bc, bp, 0), (bc, bp, -2), (bc, C.byref(params(rank=1, world=2)), 3), (bc, C.byref(params(world=2)), 3),
              (bc, C.byref(params(passes=0)), 3), (C.byref(ptamd.make_camera(1, 8)), bp, 3),
              (bc, bp, (1 << 25) // (48 * PASSES) + 1)):                                       # 64 x units reaches 2^31
        assert l.pt_views_work_bytes(*a) == -1, a
    assert l.pt_views_work_bytes(bc, bp, (1 << 25) // (48 * PASSES) - 1) > 0
    with pytest.raises(ptamd.PtError):
        ptamd.views_work_bytes(cam, prm, 0)
    with pytest.raises(ptamd.PtError):
        ptamd.views_floats(cam, 0)


def test_bad_arguments_are_rejected_before_any_device_call():
    """Fake device addresses and a fake scene: they are never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    W, H = 100, 52
    prm = params()
    bp = C.byref(prm)
    base = 1 << 40
    scene, d_tiles, d_work = (C.c_void_p(base + (i << 20)) for i in range(3))
    arr = lambda cs: (ptamd.PtCamera * len(cs))(*cs)                       # noqa: E731
    fp = lambda a: ptamd._ptr(np.ascontiguousarray(a, np.int32))           # noqa: E731
    ok = arr(cams(W, H))
    other_w, other_h = cams(W, H), cams(W, H)
    other_w[1].W = W + 8
    other_h[2].H = H - 1
    last_ok = SEED_LIMIT // (W * H) - PASSES                               # the largest first pass whose seeds still fit
    rgb = np.zeros((3, H, W, 3), np.float32)
    cases = [
        ("NULL scene", (None, ok, 3, bp, None)),
        ("NULL cameras", (scene, None, 3, bp, None)),
        ("NULL params", (scene, ok, 3, None, None)),
        ("n_views = 0", (scene, ok, 0, bp, None)),
        ("n_views < 0", (scene, ok, -3, bp, None)),
        ("unequal W", (scene, arr(other_w), 3, bp, None)),
        ("unequal H", (scene, arr(other_h), 3, bp, None)),
        ("W < 2", (scene, arr([ptamd.make_camera(1, 8)] * 3), 3, bp, None)),
        ("world = 2", (scene, ok, 3, C.byref(params(rank=0, world=2)), None)),
        ("rank 1 of 2", (scene, ok, 3, C.byref(params(rank=1, world=2)), None)),
        ("negative first_pass", (scene, ok, 3, bp, fp([0, -1, 4]))),
        ("seed overflow in one view", (scene, ok, 3, bp, fp([0, last_ok + 1, 4]))),
        ("seed overflow through prm", (scene, ok, 3, C.byref(params(first_pass=last_ok + 1)), None)),
        ("passes = 0", (scene, ok, 3, C.byref(params(passes=0)), None)),
        ("spp = 0", (scene, ok, 3, C.byref(params(spp_per_pass=0)), None)),
    ]
    for what, (s, c, n, p, f) in cases:
        assert l.pt_render_views(s, c, n, p, f, d_tiles, d_work, None) == -1, what
        assert l.pt_last_error(), what
        assert l.pt_render_views_host(s, c, n, p, f, ptamd._ptr(rgb)) == -1, what
    assert l.pt_render_views(scene, ok, 3, bp, None, None, d_work, None) == -1
    assert l.pt_render_views(scene, ok, 3, bp, None, d_tiles, None, None) == -1
    assert l.pt_render_views_host(scene, ok, 3, bp, None, None) == -1
    # too many streams for one pipeline run: 64 x (views x tiles x passes) must stay below 2^31 (bit 31 of a queue entry is the resume flag)
    many = (1 << 25) // (n_tiles_of(W, H) * PASSES) + 1
    big = arr([ptamd.make_camera(W, H)] * many)
    assert l.pt_render_views(scene, big, many, bp, None, d_tiles, d_work, None) == -1
    assert "2^31" in l.pt_last_error().decode()
    l.pt_render_views(scene, arr(other_w), 3, bp, None, d_tiles, d_work, None)
    assert "view 1" in l.pt_last_error().decode()
    l.pt_render_views(scene, ok, 3, bp, fp([0, last_ok + 1, 4]), d_tiles, d_work, None)
    assert "overflows" in l.pt_last_error().decode()
    # the wrapper checks what ctypes cannot
    with pytest.raises(ptamd.PtError):
        ptamd.Scene.render_views(None, [], prm)
    with pytest.raises(ptamd.PtError):
        ptamd.Scene.render_views(None, cams(W, H), prm, first_pass=[0, 1])


def test_cli_lists_the_options_and_names_a_bad_line(tmp_path):
    r = subprocess.run([PTRENDER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("--cam-pos", "--cam-rot", "--fov", "--views"):
        assert opt in r.stdout, opt
    good = "0 20 60 0 90 0 45\n# a comment\n\n0 20 53  0 93.5 0  45  5   # trailing comment\n"
    for bad_line in ("14 23.5 60 0 97 0\n", "14 23.5 60 0 97 0 35 2 9\n", "14 23.5 sixty 0 97 0 35\n", "14 23.5 60 0 97 0 0\n", "14 23.5 60 0 97 0 35 -1\n"):
        f = tmp_path / "views.txt"
        f.write_text(good + bad_line)
        r = subprocess.run([PTRENDER, "--views", str(f), "--width", "64", "--height", "48"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and "line 5" in r.stderr, (bad_line, r.stderr)
    f.write_text("# nothing\n")
    assert subprocess.run([PTRENDER, "--views", str(f)], capture_output=True, timeout=60, cwd=tmp_path).returncode == 2
    assert subprocess.run([PTRENDER, "--views", str(tmp_path / "missing.txt")], capture_output=True, timeout=60, cwd=tmp_path).returncode == 2
    f.write_text(good)
    v = ["--views", str(f)]
    for bad in (v + ["--window", "8,8,40,24"], v + ["--world", "2", "--rank", "0", "--id-file", "job.id"], v + ["--target-error", "0.1"],
                v + ["--denoise", "d.png"], v + ["--aov", "a.bin"], ["--fov", "0"], ["--fov", "180"], ["--cam-pos", "1,2"], ["--cam-rot", "1"]):
        r = subprocess.run([PTRENDER, "--width", "64", "--height", "48"] + bad, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    import oracle_lib as O
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    O.set_libm(1)            # the pinned contract: correctly rounded float transcendentals
    yield


def _build(name):
    """(nodes, tris, spheres) of a test scene."""
    prims = ptamd.gen_scene(0, 187) if name == "cornell" else ptamd.gen_scene(1, 16)
    nodes, tris, _ = ptamd.build_bvh(prims)
    return nodes, tris, (make_test_spheres() if name == "standin_spheres" else None)


def _scene(name):
    nodes, tris, sph = _build(name)
    return ptamd.Scene(nodes, tris, sph)


def _singles(sc, cs, prm, first=None):
    """The yardstick: one pt_render per camera (with its own first pass where given)."""
    out = []
    for v, cam in enumerate(cs):
        p = ptamd.PtParams.from_buffer_copy(prm)
        if first is not None:
            p.first_pass = int(first[v])
        out.append(sc.render(cam, p))
    return np.stack(out)


def _assert_same(got, want, what):
    same = (bits(got) == bits(want))
    print(f"{what}: bit-identical floats {same.mean():.6f}")
    assert got.shape == want.shape and same.all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "standin", "standin_spheres"])
def test_every_view_is_the_single_render(_gpu, name):
    sc = _scene(name)
    for W, H in FRAMES:
        cs = cams(W, H)
        for prm in (params(),) + ((params(max_bounce=12),) if (W, H) == FRAMES[0] else ()):
            want = _singles(sc, cs, prm)
            assert np.isfinite(want).all() and want.mean() > 0.05
            assert not np.array_equal(bits(want[0]), bits(want[1])) and not np.array_equal(bits(want[0]), bits(want[2]))
            got = sc.render_views(cs, prm)
            assert got.dtype == np.float32
            _assert_same(got, want, f"{name} {W}x{H} max_bounce {prm.max_bounce}")
            for order in ((2, 0, 1), (1, 1, 0), (2, 2, 2, 0), (1,), (2,)):      # shuffled, a camera listed twice, one view alone
                _assert_same(sc.render_views([cs[i] for i in order], prm), want[list(order)], f"{name} {W}x{H} order {order}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "standin"])
def test_every_view_is_the_oracles_render(_gpu, name):
    import oracle_lib as O
    nodes, tris, _ = _build(name)
    so, sg = O.Scene(nodes.tobytes(), tris), ptamd.Scene(nodes, tris)
    W, H = FRAMES[0]
    prm = params()
    got = sg.render_views(cams(W, H), prm)
    for v, (pos, rot, fov) in enumerate(CAMERAS):
        ref, _ = so.render(O.make_camera(W, H, pos=pos, rot=rot, fovy_deg=fov), O.make_params(W, H, prm.passes, prm.spp_per_pass), 16)
        assert np.isfinite(ref).all()
        _assert_same(got[v], ref, f"{name} view {v} against the oracle")


@pytest.mark.gpu
def test_first_pass_per_view(_gpu):
    sc = _scene("standin")
    for W, H in FRAMES:
        cs, prm = cams(W, H), params(first_pass=2)
        first = [0, 5, 9]
        want = _singles(sc, cs, prm, first)
        _assert_same(sc.render_views(cs, prm, first_pass=first), want, f"{W}x{H} first_pass {first}")
        assert not np.array_equal(bits(want), bits(_singles(sc, cs, prm)))
        # NULL = prm->first_pass for every view
        _assert_same(sc.render_views(cs, prm), sc.render_views(cs, prm, first_pass=[2, 2, 2]), f"{W}x{H} NULL first_pass")
        _assert_same(sc.render_views(cs, prm), _singles(sc, cs, prm), f"{W}x{H} prm.first_pass")


_EARLY_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
import ptamd
from test_views import cams, params, _scene, FRAMES
W, H = FRAMES[0]
sc = _scene("standin_spheres")
out = []
for rounds in (1, 0):
    sc.set_shade_rounds(rounds)
    sc.set_early_shade(int(sys.argv[3]))
    out.append(sc.render_views(cams(W, H), params()))
np.save(sys.argv[4], np.stack(out))
"""


@pytest.mark.gpu
def test_schedules_and_thresholds_are_result_neutral(_gpu, tmp_path):
    """pt_set_shade_rounds, pt_set_drain_threshold and pt_set_early_shade choose among the views instantiations of wf_shade and
    wf_drain: every choice gives the bits of the single renders.  That the early-shade phases really ran is read off a kernel trace."""
    sc = _scene("standin_spheres")
    W, H = FRAMES[0]
    cs, prm = cams(W, H), params()
    want = _singles(sc, cs, prm)
    streams = len(cs) * n_tiles_of(W, H) * 64 * prm.passes      # the batch's own stream count
    assert streams == 27648
    for rounds in (0, 1, -1):
        sc.set_shade_rounds(rounds)
        for drain in (0, streams + 1, 80000 // 64):
            sc.set_drain_threshold(drain)
            _assert_same(sc.render_views(cs, prm), want, f"rounds {rounds} drain {drain}")
        sc.set_drain_threshold(80000)
        for early in (streams, streams * 8, 0, streams - 1, streams * 8 + 8):      # on / on / never / off (too many streams) / off (too few)
            sc.set_early_shade(early)
            sc.set_drain_threshold(0 if early == streams else 80000)              # once with the early phases to the last stream
            _assert_same(sc.render_views(cs, prm), want, f"rounds {rounds} early {early}")
        sc.set_early_shade(2500000)
    # the early phases under a kernel trace, in a process of its own
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    assert os.path.exists(prof), "rocprofv3 is needed to see which kernels ran"
    script, frames, outdir = tmp_path / "early_child.py", tmp_path / "frames.npy", tmp_path / "trace"
    script.write_text(_EARLY_CHILD)
    r = subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(outdir), "--", sys.executable, str(script),
                        os.path.join(ROOT, "pathtrace-on-cuda_amd"), os.path.join(ROOT, "tests"), str(streams), str(frames)],
                       capture_output=True, text=True, timeout=900, cwd=tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(frames)
    _assert_same(got[0], want, "traced, two rounds per step")
    _assert_same(got[1], want, "traced, one bounce per step")
    text = ""
    for d, _, files in os.walk(outdir):
        for f in files:
            if f.endswith(".csv"):
                text += open(os.path.join(d, f)).read()
    # wf_shade<WAVES, TWO, PHASE, MARK, Cam>: a batch runs the Cam = ptd::ViewTable instantiations (4 waves per SIMD), never a ptd::DevCamera one
    shades = set(re.findall(r"wf_shade<[^>]*>", text))
    print("shade kernels in the trace:", sorted(shades))
    for two in ("true", "false"):
        for phase in (1, 2):
            assert f"wf_shade<4, {two}, {phase}, true, ptd::ViewTable>" in shades, (two, phase, sorted(shades))
    assert "wf_init_views" in text and all(k.endswith(", ptd::ViewTable>") for k in shades), sorted(shades)


class Device:
    """torch buffers for the device-pointer calls; everything on one stream."""

    def __init__(self, sc):
        import torch
        self.torch, self.sc = torch, sc
        self.dev = torch.device("cuda:0")
        self.stream = torch.cuda.Stream(self.dev)

    def _host(self, tiles, work, shape_t, shape_w):
        t = self.torch
        with t.cuda.stream(self.stream):
            slab = work[:int(np.prod(shape_w)) * 4].view(t.float32).cpu().numpy().reshape(shape_w)
            out = tiles.cpu().numpy().reshape(shape_t)
        self.stream.synchronize()
        return out, slab

    def single(self, cam, prm):
        """pt_render_tiles(world 1): (tiles (n, 192), per-pass means (passes, n, 192))."""
        t, n = self.torch, n_tiles_of(cam.W, cam.H)
        tiles = t.empty(ptamd.tiles_floats(cam, prm), dtype=t.float32, device=self.dev)
        work = t.empty(ptamd.work_bytes(cam, prm), dtype=t.uint8, device=self.dev)
        self.sc.render_tiles(cam, prm, tiles.data_ptr(), work.data_ptr(), self.stream.cuda_stream)
        return self._host(tiles, work, (n, 192), (prm.passes, n, 192))

    def batch(self, cs, prm, first=None):
        """pt_render_views with buffers of exactly pt_views_floats / pt_views_work_bytes: (tiles (V, n, 192), means (passes, V, n, 192))."""
        t, n, V = self.torch, n_tiles_of(cs[0].W, cs[0].H), len(cs)
        tiles = t.empty(ptamd.views_floats(cs[0], V), dtype=t.float32, device=self.dev)
        work = t.empty(ptamd.views_work_bytes(cs[0], prm, V), dtype=t.uint8, device=self.dev)
        self.sc.render_views_device(cs, prm, tiles.data_ptr(), work.data_ptr(), self.stream.cuda_stream, first_pass=first)
        return self._host(tiles, work, (V, n, 192), (prm.passes, V, n, 192)) + (tiles,)

    def untile(self, tiles, v, cam):
        t = self.torch
        per = ptamd.views_floats(cam, 1)
        with t.cuda.stream(self.stream):
            frame = t.empty((cam.H, cam.W, 3), dtype=t.float32, device=self.dev)
        ptamd.untile(tiles.data_ptr() + 4 * per * v, cam, 1, frame.data_ptr(), self.stream.cuda_stream)
        with t.cuda.stream(self.stream):
            h = frame.cpu().numpy()
        self.stream.synchronize()
        return h


@pytest.mark.gpu
def test_work_buffer_holds_the_per_pass_means_view_major(_gpu):
    sc = _scene("standin")
    dv = Device(sc)
    for W, H in FRAMES:
        cs, prm, first = cams(W, H), params(first_pass=1), [1, 4, 0]
        got, slab, d_tiles = dv.batch(cs, prm, first)
        for v, cam in enumerate(cs):
            p = params(first_pass=first[v])
            want, want_slab = dv.single(cam, p)
            _assert_same(got[v], want, f"{W}x{H} tiles of view {v}")
            _assert_same(slab[:, v], want_slab, f"{W}x{H} means of view {v}")
            S, _ = fold(slab[:, v])
            _assert_same(S, got[v], f"{W}x{H} fold of view {v}")
            # pt_untile on the view's slice assembles its frame
            _assert_same(dv.untile(d_tiles, v, cam), sc.render(cam, p), f"{W}x{H} untile of view {v}")
        # padding pixels of ragged tiles are exactly 0 (positive zero)
        last = got[:, -1].reshape(len(cs), 8, 8, 3)
        vh, vw = H - (H - 1) // 8 * 8, W - (W - 1) // 8 * 8
        assert not bits(last[:, vh:]).any() and not bits(last[:, :, vw:]).any()


@pytest.mark.gpu
def test_batch_has_no_side_effects_and_ignores_the_mode(_gpu):
    sc = _scene("standin")
    W, H = FRAMES[1]
    cs, prm = cams(W, H), params()
    win = (5, 3, 37, 29)
    before, before_win = sc.render(cs[0], prm), sc.render_window(cs[0], prm, win)
    want = _singles(sc, cs, prm)
    _assert_same(sc.render_views(cs, prm), want, "batch")
    _assert_same(sc.render(cs[0], prm), before, "pt_render after a batch")
    _assert_same(sc.render_window(cs[0], prm, win), before_win, "pt_render_tile_list after a batch")
    sc.set_mode(0)
    mode0 = sc.render(cs[0], prm)
    _assert_same(mode0, before, "mode 0")
    _assert_same(sc.render_views(cs, prm), want, "batch with mode 0 set")
    sc.render_timings(reset=True)
    _assert_same(sc.render(cs[0], prm), before, "mode 0 after a batch")
    assert sc.render_timings(reset=False).size == 1             # ... and that render was one render_units launch: mode 0 is still set
    sc.set_mode(1)
    # the scene-owned camera buffers grow and shrink: many views, then few, then many again
    many = [cs[i % 3] for i in range(70)]
    for group in (many, cs[:2], many[:67], cs[2:]):
        got = sc.render_views(group, prm)
        idx = [next(i for i in range(3) if c is cs[i]) for c in group]
        _assert_same(got, want[idx], f"{len(group)} views")
    assert sc.last_iterations() > 0
    assert sc.last_render_ms() > 0.0
    _assert_same(sc.render(cs[0], prm), before, "pt_render at the end")


@pytest.mark.gpu
def test_cli_views(_gpu, tmp_path):
    W, H = 100, 52
    args = [PTRENDER, "--scene", "standin", "--lat-lon", "16", "--width", str(W), "--height", str(H), "--passes", "2", "--spp", "3"]
    run = lambda extra, d: subprocess.run(args + extra, cwd=d, check=True, capture_output=True, timeout=300, text=True)      # noqa: E731
    batch = tmp_path / "batch"
    batch.mkdir()
    lines = ["# px py pz rx ry rz fov [first_pass]"] + [f"{p[0]} {p[1]} {p[2]} {r[0]} {r[1]} {r[2]} {f}" for p, r, f in CAMERAS]
    (batch / "views.txt").write_text("\n".join(lines) + "\n")
    run(["--views", "views.txt", "--raw", "r.bin"], batch)
    assert not (batch / "result.png").exists()
    for v, (p, r, f) in enumerate(CAMERAS):
        d = tmp_path / f"single{v}"
        d.mkdir()
        run(["--cam-pos", f"{p[0]},{p[1]},{p[2]}", "--cam-rot", f"{r[0]},{r[1]},{r[2]}", "--fov", str(f), "--raw", "r.bin"], d)
        assert (batch / f"result_{v:03d}.png").read_bytes() == (d / "result.png").read_bytes(), v
        raw = np.fromfile(batch / f"r.bin_{v:03d}", np.float32)
        assert raw.size == W * H * 3 and np.array_equal(bits(raw), bits(np.fromfile(d / "r.bin", np.float32))), v
    assert (batch / "result_000.png").read_bytes() != (batch / "result_001.png").read_bytes()
    # no new option = the reference application's camera spelled out
    plain = tmp_path / "plain"
    plain.mkdir()
    run([], plain)
    assert (plain / "result.png").read_bytes() == (tmp_path / "single0" / "result.png").read_bytes()
    # a first pass per line
    fp = tmp_path / "fp"
    fp.mkdir()
    (fp / "views.txt").write_text("0 20 60 0 90 0 45 0\n0 20 60 0 90 0 45 7\n")
    run(["--views", "views.txt"], fp)
    assert (fp / "result_000.png").read_bytes() == (plain / "result.png").read_bytes()
    assert (fp / "result_001.png").read_bytes() != (plain / "result.png").read_bytes()
