"""Radiance along the caller's own rays (pt_render_rays, pt_render_rays_host, pt_rays_floats, pt_rays_work_bytes, ptamd.camera_rays,
ptamd.equirect_rays): the C-ABI surface, the sizes and the argument checks on the CPU; on the GPU equality of bits with the camera
render whose rays they are (frames, cameras, passes, any order and explicit seeds, the per-pass means, schedules and hand-over
thresholds, side effects, stream order with a vertex update), the meaning of tmax, and the CPU oracle's render as the check that is not
the code under test.  Bits everywhere, no tolerances."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import dynamic_ref as R
import ptamd
from stats_ref import fold
from test_views import CAMERAS, FRAMES, _assert_same, _build, _scene, bits, cams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pt_rays_floats", "pt_rays_work_bytes", "pt_render_rays", "pt_render_rays_host")
SPP = 4


def params(**kw):
    return ptamd.default_params(**{**dict(passes=1, spp_per_pass=SPP), **kw})


def groups_of(n):
    return (n + 63) // 64


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: C-ABI surface, sizes, argument checks, the panorama helper (no device is touched)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound():
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in NEW_SYMBOLS:
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    for name in ("render_rays", "render_rays_device"):
        assert callable(getattr(ptamd.Scene, name))
    for name in ("rays_floats", "rays_work_bytes", "camera_rays", "equirect_rays"):
        assert callable(getattr(ptamd, name))


def test_rays_floats_is_whole_groups_of_64():
    for n, want in ((1, 192), (63, 192), (64, 192), (65, 384), (5200, 192 * 82)):
        assert ptamd.rays_floats(n) == want == 192 * groups_of(n), n
    l = ptamd.lib()
    for n in (0, -1, -(1 << 40)):
        assert l.pt_rays_floats(n) == -1, n
    with pytest.raises(ptamd.PtError):
        ptamd.rays_floats(0)


def test_work_bytes_are_those_of_a_frame_with_as_many_tiles():
    l = ptamd.lib()
    for n in (1, 63, 64, 65, 5200, 1920 * 1080):
        for prm in (ptamd.default_params(passes=8), ptamd.default_params(passes=2, first_pass=3), params()):
            prm2 = ptamd.PtParams.from_buffer_copy(prm)
            prm2.first_pass, prm2.rank, prm2.world = 0, 0, 1
            assert ptamd.rays_work_bytes(prm, n) == ptamd.work_bytes(ptamd.make_camera(8 * groups_of(n), 8), prm2), (n, prm.passes)
    bp = C.byref(params(passes=3))
    for a in ((None, 64), (bp, 0), (bp, -5), (C.byref(params(rank=1, world=2)), 64), (C.byref(params(world=2)), 64), (C.byref(params(passes=0)), 64),
              (C.byref(params(spp_per_pass=65536)), 64), (bp, 64 * ((1 << 25) // 3 + 1))):      # 64 x units reaches 2^31
        assert l.pt_rays_work_bytes(*a) == -1, a
    assert l.pt_rays_work_bytes(bp, 64 * ((1 << 25) // 3)) > 0
    with pytest.raises(ptamd.PtError):
        ptamd.rays_work_bytes(params(), 0)


def test_bad_arguments_are_rejected_before_any_device_call():
    """Fake device addresses and a fake scene: they are never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    n = 5200
    bp = C.byref(params(passes=3))
    base = 1 << 40
    scene, d_rays, d_seed, d_rgb, d_work = (C.c_void_p(base + (i << 24)) for i in range(5))
    h_rays, h_rgb = np.zeros((n, 8), np.float32), np.zeros((n, 3), np.float32)
    too_many = 64 * ((1 << 25) // 3 + 1)
    # (what, scene, rays, n, seed_stride, params, rgb, work)
    cases = [
        ("NULL scene", None, d_rays, n, n, bp, d_rgb, d_work),
        ("NULL rays", scene, None, n, n, bp, d_rgb, d_work),
        ("NULL params", scene, d_rays, n, n, None, d_rgb, d_work),
        ("NULL rgb", scene, d_rays, n, n, bp, None, d_work),
        ("n_rays = 0", scene, d_rays, 0, n, bp, d_rgb, d_work),
        ("n_rays < 0", scene, d_rays, -64, n, bp, d_rgb, d_work),
        ("seed_stride < 0", scene, d_rays, n, -1, bp, d_rgb, d_work),
        ("world = 2", scene, d_rays, n, n, C.byref(params(rank=0, world=2)), d_rgb, d_work),
        ("rank 1 of 2", scene, d_rays, n, n, C.byref(params(rank=1, world=2)), d_rgb, d_work),
        ("passes = 0", scene, d_rays, n, n, C.byref(params(passes=0)), d_rgb, d_work),
        ("spp = 0", scene, d_rays, n, n, C.byref(params(spp_per_pass=0)), d_rgb, d_work),
        ("spp = 65536", scene, d_rays, n, n, C.byref(params(spp_per_pass=65536)), d_rgb, d_work),
        ("max_bounce = 0", scene, d_rays, n, n, C.byref(params(max_bounce=0)), d_rgb, d_work),
        ("max_bounce = 256", scene, d_rays, n, n, C.byref(params(max_bounce=256)), d_rgb, d_work),
        ("max_refract = -1", scene, d_rays, n, n, C.byref(params(max_refract=-1)), d_rgb, d_work),
        ("max_refract = 251", scene, d_rays, n, n, C.byref(params(max_refract=251)), d_rgb, d_work),
        ("64 x units reaches 2^31", scene, d_rays, too_many, n, bp, d_rgb, d_work),
    ]
    for what, s, r, k, stride, p, rgb, w in cases:
        for seed in (None, d_seed):
            assert l.pt_render_rays(s, r, seed, k, stride, p, rgb, w, None) == -1, what
            assert l.pt_last_error(), what
        hr = None if r is None else ptamd._ptr(h_rays)
        ho = None if rgb is None else ptamd._ptr(h_rgb)
        assert l.pt_render_rays_host(s, hr, None, k, stride, p, ho) == -1, what
        assert l.pt_last_error(), what
    # what only the device call has: the work buffer and the alignment of its pointers
    for what, r, rgb, w in (("NULL work", d_rays, d_rgb, None), ("rays 8 bytes off", C.c_void_p(d_rays.value + 8), d_rgb, d_work),
                            ("rays 4 bytes off", C.c_void_p(d_rays.value + 4), d_rgb, d_work), ("rgb 8 bytes off", d_rays, C.c_void_p(d_rgb.value + 8), d_work),
                            ("rgb 4 bytes off", d_rays, C.c_void_p(d_rgb.value + 4), d_work)):
        assert l.pt_render_rays(scene, r, None, n, n, bp, rgb, w, None) == -1, what
        assert l.pt_last_error(), what
    l.pt_render_rays(scene, d_rays, None, too_many, n, bp, d_rgb, d_work, None)
    assert "2^31" in l.pt_last_error().decode()
    l.pt_render_rays(scene, C.c_void_p(d_rays.value + 8), None, n, n, bp, d_rgb, d_work, None)
    assert "aligned" in l.pt_last_error().decode()
    # the wrapper checks what ctypes cannot
    with pytest.raises(ptamd.PtError):
        ptamd.Scene.render_rays(None, np.zeros((4, 6), np.float32), params())
    with pytest.raises(ptamd.PtError):
        ptamd.Scene.render_rays(None, np.zeros((4, 8), np.float32), params(), seeds=[1, 2, 3])
    with pytest.raises(ptamd.PtError):
        ptamd.Scene.render_rays(None, [[0.0] * 8], params())


def test_equirect_rays_cover_the_sphere_with_unit_directions():
    pos = (1.5, -2.0, 3.25)
    for W, H in ((9, 5), (64, 32), (101, 37)):
        r = ptamd.equirect_rays(pos, W, H)
        assert r.shape == (W * H, 8) and r.dtype == np.float32
        assert np.array_equal(r[:, 0:3], np.broadcast_to(np.float32(pos), (W * H, 3)))
        assert not r[:, 6].any() and (r[:, 7] == np.float32(999999.0)).all()
        d = r[:, 3:6].astype(np.float64)
        # float32 components of a unit vector: each is off by at most half an ulp (2^-24 relative), so is the length to first order
        assert np.abs(np.sqrt((d * d).sum(1)) - 1.0).max() <= 2.0 ** -23
        img = r[:, 3:6].reshape(H, W, 3)
        assert (img[0, :, 1] > 0).all() and (img[-1, :, 1] < 0).all()                  # row 0 is nearest +y
        assert (img[:, W // 2 + 1:, 0] > 0).all() and (img[:, :(W - 1) // 2, 0] < 0).all()      # x grows to the right (+x)
        if W % 2 and H % 2:
            assert np.abs(img[H // 2, W // 2] - np.float32([0, 0, -1])).max() <= 2.0 ** -23, (W, H)      # the centre pixel looks down -z
        else:
            mid = img[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1].astype(np.float64).sum((0, 1))
            assert np.abs(mid / np.linalg.norm(mid) - [0, 0, -1]).max() <= 1e-6, (W, H)
        # the directions cover the sphere evenly: weighted by the solid angle of a pixel they sum to nothing
        w = np.sin(np.pi * (np.arange(H) + 0.5) / H)[:, None, None]
        assert np.abs((img.astype(np.float64) * w).sum((0, 1))).max() <= 1e-4 * W * H
    with pytest.raises(ptamd.PtError):
        ptamd.equirect_rays(pos, 0, 4)


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


_rays_cache = {}


def cam_rays(W, H, which, p):
    """ptamd.camera_rays of camera `which` of test_views.CAMERAS, computed once per (frame, camera, pass) and never written to."""
    key = (W, H, which, p)
    if key not in _rays_cache:
        rays, seeds, stride = ptamd.camera_rays(cams(W, H, (which,))[0], p)
        rays.setflags(write=False)
        seeds.setflags(write=False)
        _rays_cache[key] = (rays, seeds, stride)
    return _rays_cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "standin", "standin_spheres"])
def test_a_cameras_rays_are_the_cameras_frame(_gpu, name):
    sc = _scene(name)
    for W, H in FRAMES:
        for which in (0, 1, 2):
            cam = cams(W, H, (which,))[0]
            for p in (0, 2):
                prm = params(first_pass=p)
                want = sc.render(cam, prm)
                assert np.isfinite(want).all() and want.mean() > 0.01
                rays, seeds, stride = cam_rays(W, H, which, p)
                assert rays.shape == (W * H, 8) and stride == W * H
                got = sc.render_rays(rays, prm, seeds, stride)
                assert got.dtype == np.float32 and got.shape == (W * H, 3)
                _assert_same(got.reshape(H, W, 3), want, f"{name} {W}x{H} camera {which} pass {p}")
    # seeds = None is ray i seeded with i, the stride defaults to n: the camera's own numbering
    W, H = FRAMES[1]
    rays, seeds, stride = cam_rays(W, H, 0, 2)
    assert np.array_equal(seeds, np.arange(W * H)) and stride == W * H
    _assert_same(sc.render_rays(rays, params(first_pass=2)).reshape(H, W, 3), sc.render(cams(W, H, (0,))[0], params(first_pass=2)), f"{name} default seeds")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "standin"])
def test_against_the_oracles_render(_gpu, name):
    import oracle_lib as O
    nodes, tris, _ = _build(name)
    so, sg = O.Scene(nodes.tobytes(), tris), ptamd.Scene(nodes, tris)
    W, H = FRAMES[0]
    pos, rot, fov = CAMERAS[0]
    ocam = O.make_camera(W, H, pos=pos, rot=rot, fovy_deg=fov)
    py, px = np.divmod(np.arange(W * H, dtype=np.int32), np.int32(W))
    for p in (0, 2):
        out8 = O.pixel_dir(ocam, np.stack([px, py, np.full(W * H, p, np.int32)], 1))
        rays = np.zeros((W * H, 8), np.float32)
        rays[:, 0:3] = np.float32(pos)
        rays[:, 3:6] = out8[:, 2:5]
        rays[:, 7] = 999999.0
        got = sg.render_rays(rays, params(first_pass=p), py * W + px, W * H)
        ref, _ = so.render(ocam, O.make_params(W, H, 1, SPP, first_pass=p), 16)
        assert np.isfinite(ref).all() and ref.mean() > 0.01
        _assert_same(got.reshape(H, W, 3), ref, f"{name} pass {p} against the oracle")


@pytest.mark.gpu
def test_any_origin_any_order_explicit_seeds(_gpu):
    sc = _scene("standin_spheres")
    W, H = FRAMES[1]
    p = 1
    prm = params(first_pass=p)
    frames = sc.render_views(cams(W, H), prm).reshape(-1, 3)                    # the three cameras' single-pass frames, pixel-major
    parts = [cam_rays(W, H, which, p) for which in (0, 1, 2)]
    rays, seeds = np.concatenate([r for r, _, _ in parts]), np.concatenate([s for _, s, _ in parts])
    stride = W * H
    perm = np.random.RandomState(20240517).permutation(len(rays))
    n = 64 * 150 + 37
    assert n < len(rays) and n % 64 == 37
    pick = perm[:n]
    assert len({tuple(o) for o in rays[pick, 0:3]}) == 3                        # origins of all three cameras, mixed
    got = sc.render_rays(rays[pick], prm, seeds[pick], stride)
    _assert_same(got, frames[pick], f"{n} permuted rays of three cameras")
    for k in (1, 63, 64, 65):
        pick = perm[n:n + k]
        _assert_same(sc.render_rays(rays[pick], prm, seeds[pick], stride), frames[pick], f"{k} rays")


class Device:
    """torch buffers for the device-pointer call; everything on one stream."""

    def __init__(self, sc):
        import torch
        self.torch, self.sc = torch, sc
        self.dev = torch.device("cuda:0")
        self.stream = torch.cuda.Stream(self.dev)

    def render(self, rays, prm, seeds, stride):
        """pt_render_rays with buffers of exactly pt_rays_floats / pt_rays_work_bytes: (d_rgb (floats,), means (passes, floats), work)."""
        t, n = self.torch, len(rays)
        with t.cuda.stream(self.stream):
            d_rays, d_seed = t.from_numpy(np.array(rays)).to(self.dev), t.from_numpy(np.array(seeds)).to(self.dev)
            rgb = t.empty(ptamd.rays_floats(n), dtype=t.float32, device=self.dev)
            work = t.empty(ptamd.rays_work_bytes(prm, n), dtype=t.uint8, device=self.dev)
            self.sc.render_rays_device(d_rays.data_ptr(), n, prm, rgb.data_ptr(), work.data_ptr(), d_seed.data_ptr(), stride, self.stream.cuda_stream)
            slab = work[:prm.passes * rgb.numel() * 4].view(t.float32).cpu().numpy().reshape(prm.passes, -1)
            out = rgb.cpu().numpy()
        self.stream.synchronize()
        return out, slab, work


@pytest.mark.gpu
def test_passes_and_the_work_buffers_means(_gpu):
    import torch
    sc = _scene("standin")
    dv = Device(sc)
    W, H = FRAMES[1]
    n, first, passes = W * H, 1, 3
    assert n == 5200 and n % 64 == 16
    rays, seeds, stride = cam_rays(W, H, 0, 0)
    prm = params(passes=passes, first_pass=first)
    rgb, slab, d_work = dv.render(rays, prm, seeds, stride)
    floats = ptamd.rays_floats(n)
    assert rgb.shape == (floats,) and slab.shape == (passes, floats)
    for k in range(passes):
        one = sc.render_rays(rays, params(first_pass=first + k), seeds, stride)
        _assert_same(slab[k, :3 * n].reshape(n, 3), one, f"means of pass {first + k}")
    assert not np.array_equal(bits(slab[0]), bits(slab[1])) and not np.array_equal(bits(slab[1]), bits(slab[2]))
    S, _ = fold(slab)
    _assert_same(rgb, S, "d_rgb is ((0 + m0) + m1) + m2")
    # the padding rays of the last group are exactly +0, in the sum and in every pass
    assert floats - 3 * n == 3 * 48
    assert not bits(rgb[3 * n:]).any() and not bits(slab[:, 3 * n:]).any()
    # pt_accumulate_passes reads the slab as that of a frame of 8 G x 8 pixels
    cam8 = ptamd.make_camera(8 * groups_of(n), 8)
    prm8 = params(passes=passes, first_pass=0, rank=0, world=1)
    assert ptamd.tiles_floats(cam8, prm8) == floats
    with torch.cuda.stream(dv.stream):
        mom = torch.empty((2, floats), dtype=torch.float32, device=dv.dev)
        ptamd.accumulate_passes(d_work.data_ptr(), cam8, prm8, 0, mom[0].data_ptr(), mom[1].data_ptr(), dv.stream.cuda_stream)
        h = mom.cpu().numpy()
    dv.stream.synchronize()
    S, M2 = fold(slab)
    _assert_same(h[0], rgb, "pt_accumulate_passes: S")
    _assert_same(h[1], M2, "pt_accumulate_passes: M2")


@pytest.mark.gpu
def test_tmax_ends_the_primary_ray(_gpu):
    sc = _scene("standin")
    W, H = FRAMES[0]
    rays, seeds, stride = cam_rays(W, H, 0, 0)
    prm = params()
    base = sc.render_rays(rays, prm, seeds, stride)
    t, prim = sc.trace_rays(np.array(rays))
    hit = prim >= 0
    assert hit.sum() > len(rays) // 2
    # what a pixel that looks past the scene gets: spp times radiance = 0 + 1 * 0.1 added to the pixel, then the mean
    acc = np.float32(0)
    for _ in range(SPP):
        acc = np.float32(acc + np.float32(np.float32(1) * np.float32(0.1)))
    ambient = np.float32(acc / np.float32(SPP))
    for what, cut in (("every ray that hits", hit), ("every other ray that hits", hit & (np.arange(len(rays)) % 2 == 0))):
        short = np.array(rays)
        short[cut, 7] = t[cut] * np.float32(0.5)
        got = sc.render_rays(short, prm, seeds, stride)
        _assert_same(got[cut], np.full((int(cut.sum()), 3), ambient, np.float32), f"{what}: the ambient term")
        _assert_same(got[~cut], base[~cut], f"{what}: the unchanged rays")
    assert not np.array_equal(bits(base[hit]), bits(np.full((int(hit.sum()), 3), ambient, np.float32)))
    # tmax just beyond the closest hit changes nothing
    longer = np.array(rays)
    longer[hit, 7] = t[hit] * np.float32(1.5)
    _assert_same(sc.render_rays(longer, prm, seeds, stride), base, "tmax = 1.5 t")


_SLICED_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
import ptamd
from test_rays import cam_rays, params
from test_views import _scene, FRAMES
W, H = FRAMES[0]
sc = _scene("standin")
rays, seeds, stride = cam_rays(W, H, 0, 0)
t, prim = sc.trace_rays(np.array(rays))
cut = (prim >= 0) & (np.arange(len(rays)) % 2 == 0)
short = np.array(rays)
short[cut, 7] = t[cut] * np.float32(0.5)
sc.set_drain_threshold(64 * ((len(rays) + 63) // 64) + 1)
out = sc.render_rays(short, params(), seeds, stride)
np.savez(sys.argv[3], out=out, short=short, iterations=sc.last_iterations())
"""


@pytest.mark.gpu
def test_tmax_holds_where_the_drain_kernel_traces_the_primary_ray(_gpu, tmp_path):
    """A primary ray whose time-sliced traversal is still pending when wf_drain takes over is traced again there, and must end at the
    caller's tmax there too.  A node budget of one step per launch (tuning knobs, read once per process: a child) leaves every primary
    ray pending at the first poll, where a drain threshold above the stream count hands all streams over."""
    script, out = tmp_path / "sliced_child.py", tmp_path / "sliced.npz"
    script.write_text(_SLICED_CHILD)
    env = dict(os.environ, PTAMD_BM="1", PTAMD_BS="31", PTAMD_LB="0")
    r = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "pathtrace-on-cuda_amd"), os.path.join(ROOT, "tests"), str(out)],
                       env=env, capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(out)
    assert int(got["iterations"]) == 16                          # handed over at the first poll: no ray of any depth has finished 16 node steps' worth
    W, H = FRAMES[0]
    _, seeds, stride = cam_rays(W, H, 0, 0)
    want = _scene("standin").render_rays(got["short"], params(), seeds, stride)      # the default schedule: wf_trace ends every primary ray
    _assert_same(got["out"], want, "primary rays traced by wf_drain")


_EARLY_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
import ptamd
from test_rays import cam_rays, params
from test_views import _scene, FRAMES
W, H = FRAMES[0]
sc = _scene("standin_spheres")
rays, seeds, stride = cam_rays(W, H, 0, 0)
out = []
for rounds in (1, 0):
    sc.set_shade_rounds(rounds)
    sc.set_early_shade(int(sys.argv[3]))
    out.append(sc.render_rays(rays, params(), seeds, stride))
np.save(sys.argv[4], np.stack(out))
"""


@pytest.mark.gpu
def test_schedules_and_thresholds_are_result_neutral(_gpu, tmp_path):
    """pt_set_shade_rounds, pt_set_drain_threshold and pt_set_early_shade choose among the RayTable instantiations of wf_shade and
    wf_drain: every choice gives the bits of the camera's frame.  Which kernels really ran is read off a kernel trace."""
    sc = _scene("standin_spheres")
    W, H = FRAMES[0]
    prm = params()
    want = sc.render(cams(W, H, (0,))[0], prm).reshape(-1, 3)
    rays, seeds, stride = cam_rays(W, H, 0, 0)
    streams = 64 * groups_of(len(rays)) * prm.passes
    assert streams == 3072
    for rounds in (0, 1, -1):
        sc.set_shade_rounds(rounds)
        for drain in (0, streams + 1):
            sc.set_drain_threshold(drain)
            for early in (streams, 0):
                sc.set_early_shade(early)
                _assert_same(sc.render_rays(rays, prm, seeds, stride), want, f"rounds {rounds} drain {drain} early {early}")
    # under a kernel trace, in a process of its own
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
    # wf_shade<WAVES, TWO, PHASE, MARK, Cam>: a ray render runs the Cam = ptd::RayTable instantiations, never a ptd::DevCamera or ptd::ViewTable one
    shades = set(re.findall(r"wf_shade<[^>]*>", text))
    print("shade kernels in the trace:", sorted(shades))
    for two in ("true", "false"):
        for phase in (1, 2):
            assert f"wf_shade<4, {two}, {phase}, true, ptd::RayTable>" in shades, (two, phase, sorted(shades))
    assert "wf_init_rays" in text and all(k.endswith(", ptd::RayTable>") for k in shades), sorted(shades)


@pytest.mark.gpu
def test_ray_render_has_no_side_effects_and_ignores_the_mode(_gpu):
    sc = _scene("standin")
    W, H = FRAMES[1]
    cs, prm = cams(W, H), params(passes=2)
    win = (5, 3, 37, 29)
    before, before_win, before_views = sc.render(cs[0], prm), sc.render_window(cs[0], prm, win), sc.render_views(cs, prm)
    rays, seeds, stride = cam_rays(W, H, 1, 0)
    one = params()
    want = sc.render(cs[1], one).reshape(-1, 3)
    bytes0 = sc.device_bytes
    _assert_same(sc.render_rays(rays, one, seeds, stride), want, "ray render")
    assert sc.last_iterations() > 0
    assert sc.last_render_ms() > 0.0
    assert sc.device_bytes == bytes0                                # nothing is allocated in the scene
    _assert_same(sc.render(cs[0], prm), before, "pt_render after a ray render")
    _assert_same(sc.render_window(cs[0], prm, win), before_win, "pt_render_tile_list after a ray render")
    _assert_same(sc.render_views(cs, prm), before_views, "pt_render_views after a ray render")
    sc.set_mode(0)
    _assert_same(sc.render(cs[0], prm), before, "mode 0")
    _assert_same(sc.render_rays(rays, one, seeds, stride), want, "ray render with mode 0 set")
    sc.render_timings(reset=True)
    _assert_same(sc.render(cs[0], prm), before, "mode 0 after a ray render")
    assert sc.render_timings(reset=False).size == 1             # ... and that render was one render_units launch: mode 0 is still set
    sc.set_mode(1)
    _assert_same(sc.render(cs[0], prm), before, "pt_render at the end")


@pytest.mark.gpu
def test_update_and_ray_render_in_stream_order(_gpu):
    """Update and ray render enqueued on a non-default stream with no synchronisation in between, torch tensors in and out."""
    import torch
    nodes, tris, sph = _build("standin_spheres")
    W, H = FRAMES[1]
    rays, seeds, stride = cam_rays(W, H, 0, 0)
    prm = params()
    sc = ptamd.Scene(nodes, tris, sph)
    unmoved = sc.render_rays(rays, prm, seeds, stride)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        pos = torch.from_numpy(R.positions(tris)).to(dev)
        pos = R.move_rigid_wobble(pos, torch.from_numpy(R.mesh_mask(tris)).to(dev), torch).reshape(-1, 9).contiguous()
        d_rays, d_seeds = torch.from_numpy(np.array(rays)).to(dev), torch.from_numpy(np.array(seeds)).to(dev)
        sc.update_vertices(pos, stream_ptr=st.cuda_stream)
        out = sc.render_rays(d_rays, prm, d_seeds, stride, stream_ptr=st.cuda_stream)
        assert isinstance(out, torch.Tensor) and out.device == dev and tuple(out.shape) == (len(rays), 3)
        got, h_pos = out.cpu().numpy(), pos.cpu().numpy()
    st.synchronize()
    tris2 = R.restate_tris(tris, h_pos)
    fresh = ptamd.Scene(R.refit_nodes(nodes, tris2), tris2, sph)
    _assert_same(got, fresh.render_rays(rays, prm, seeds, stride), "stream-ordered update + ray render")
    assert not np.array_equal(bits(got), bits(unmoved))
