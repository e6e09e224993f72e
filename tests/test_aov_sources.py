"""First-hit feature buffers and the denoiser for pixel windows, batches of views and the caller's rays (include/pt_api.h: the section after
"First-hit feature buffers"; csrc/pt_aov.hip).

On the CPU: the C-ABI surface, the sizes, pt_denoise_margin / pt_window_expand, every bad argument rejected before a device call, and the
cone argument on the definition (tests/denoise_ref.py): the crop of the denoise of a window grown by M = 2 (2^L - 1) equals the crop of
the full frame's denoise, and with M - 1 it does not.

On the GPU, at 100 x 52 or 64 x 48 with 2 passes, bits compared as uint32: window, view and ray feature buffers against Scene.aov,
Scene.trace_rays and the oracle, on shallow trees (the 4-wide walk) and on trees past the cut (the binary walk); stream order after an
update and a rebuild; denoise_batch against denoise per slice; the windowed denoise against the crop of the full frame's; no side effects."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_ref as D
import dynamic_ref as R
import oracle_lib as O
import ptamd
import test_deep_tree as T
from scenes_util import pinhole_rays, scene_rays8
from scenes_util import test_spheres as make_test_spheres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pt_aov_window_floats", "pt_render_aov_window", "pt_aov_window", "pt_aov_views_floats", "pt_render_aov_views", "pt_aov_views",
               "pt_aov_rays", "pt_aov_rays_host", "pt_untile_views", "pt_denoise_batch_work_bytes", "pt_denoise_batch", "pt_denoise_batch_host",
               "pt_denoise_margin", "pt_window_expand")
NEW_PYTHON = ("aov_window", "render_aov_window", "aov_views", "render_aov_views", "aov_rays", "aov_rays_device", "render_window_denoised",
              "render_views_denoised")
NEW_FUNCTIONS = ("untile_views", "denoise_batch", "denoise_batch_device", "denoise_batch_work_bytes", "denoise_margin", "expand_window",
                 "aov_window_floats", "aov_views_floats")
W, H, PASSES = 100, 52, 2      # ragged right and bottom: 13 x 7 = 91 tiles
WINDOWS = [(0, 0, 100, 52), (3, 5, 37, 29), (93, 45, 100, 52), (50, 20, 51, 21), (96, 48, 100, 52)]
DN_WINDOWS = [(40, 20, 60, 32), (0, 0, 20, 12)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """Every float has the same bits, or is a NaN on both sides (so the non-finite positions are equal)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def crop(a, win, origin=(0, 0)):
    x0, y0, x1, y1 = win
    return a[y0 - origin[1]:y1 - origin[1], x0 - origin[0]:x1 - origin[0]]


def expand(win, m, w, h):
    """pt_window_expand in three lines of numpy."""
    lo = np.maximum(np.array(win[:2], np.int64) - m, 0)
    hi = np.minimum(np.array(win[2:], np.int64) + m, [w, h])
    return tuple(int(v) for v in np.concatenate([lo, hi]))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the C-ABI surface (no device is touched) and the cone argument on the definition
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound():
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in NEW_SYMBOLS:
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    for name in NEW_PYTHON:
        assert callable(getattr(ptamd.Scene, name)), name
    for name in NEW_FUNCTIONS:
        assert callable(getattr(ptamd, name)), name
    for retired in ("No list variants of pt_render_aov", "view variants of pt_render_aov", "AOVs or the denoiser on a ray batch"):
        assert retired not in hdr, retired


def test_float_and_byte_counts():
    l = ptamd.lib()
    cam = ptamd.make_camera(W, H)
    for x0, y0, x1, y1 in WINDOWS:
        assert ptamd.aov_window_floats(cam, (x0, y0, x1, y1)) == (y1 - y0) * (x1 - x0) * 8
    for bad in ((-1, 0, 10, 10), (0, 0, 101, 52), (0, 0, 100, 53), (10, 10, 10, 20), (10, 10, 20, 9), (0, -2, 5, 5)):
        assert l.pt_aov_window_floats(C.byref(cam), *bad) == -1, bad
    assert l.pt_aov_window_floats(None, 0, 0, 1, 1) == -1 and l.pt_aov_window_floats(C.byref(ptamd.make_camera(1, 5)), 0, 0, 1, 1) == -1
    for n in (1, 3, 16):
        assert ptamd.aov_views_floats(cam, n) == n * W * H * 8
        assert ptamd.denoise_batch_work_bytes(W, H, n) == 48 * W * H * n
    assert ptamd.denoise_batch_work_bytes(W, H, 1) == ptamd.denoise_work_bytes(W, H)
    assert ptamd.denoise_batch_work_bytes(64, 64, 65535) == 48 * 64 * 64 * 65535
    assert l.pt_aov_views_floats(C.byref(cam), 0) == -1 and l.pt_aov_views_floats(None, 2) == -1
    assert l.pt_aov_views_floats(C.byref(ptamd.make_camera(4096, 4096)), 16) == 16 * 4096 * 4096 * 8      # 2^28 pixels: the limit
    assert l.pt_aov_views_floats(C.byref(ptamd.make_camera(4096, 4096)), 17) == -1
    for w, h, n in ((1, 5, 1), (5, 1, 1), (8, 8, 0), (8, 8, -1), (8, 8, 65536), (4096, 4096, 17)):
        assert l.pt_denoise_batch_work_bytes(w, h, n) == -1, (w, h, n)


def test_denoise_margin_is_the_sum_of_the_reaches():
    l = ptamd.lib()
    for L in range(13):
        assert l.pt_denoise_margin(L) == 2 * (2 ** L - 1) == sum(2 * 2 ** i for i in range(L)) == ptamd.denoise_margin(L)
    for L in (-1, 13, 100, -(2 ** 31)):
        assert l.pt_denoise_margin(L) == -1, L
    assert ptamd.denoise_margin() == 62 == ptamd.denoise_margin(D.DEFAULTS["iterations"])
    with pytest.raises(ptamd.PtError):
        ptamd.denoise_margin(13)


def test_window_expand_is_three_lines_of_numpy():
    cam = ptamd.make_camera(W, H)
    M = ptamd.denoise_margin()
    cases = [((40, 20, 60, 32), 14), ((40, 20, 60, 32), 0), ((40, 20, 60, 32), -1), ((0, 0, W, H), 5), ((0, 0, W, H), 0), ((0, 0, 20, 12), 6),
             ((3, 5, 37, 29), 8), ((93, 45, 100, 52), 30), ((50, 20, 51, 21), 1), ((50, 20, 51, 21), 2 ** 31 - 1)]
    for win, m in cases:
        assert ptamd.expand_window(cam, win, m) == expand(win, M if m == -1 else m, W, H), (win, m)
    assert ptamd.expand_window(cam, (0, 0, 20, 12), 6) == (0, 0, 26, 18)                      # clipped at two sides
    assert ptamd.expand_window(cam, (40, 20, 60, 32)) == (0, 0, 100, 52)                      # margin -1 = 62 swallows this frame
    assert ptamd.expand_window(ptamd.make_camera(1920, 1080), (800, 400, 1056, 656)) == (738, 338, 1118, 718)
    l = ptamd.lib()
    win, out = (C.c_int32 * 4)(40, 20, 60, 32), (C.c_int32 * 4)()
    assert l.pt_window_expand(None, C.byref(win), 0, C.byref(out)) == -1
    assert l.pt_window_expand(C.byref(cam), None, 0, C.byref(out)) == -1
    assert l.pt_window_expand(C.byref(cam), C.byref(win), 0, None) == -1
    assert l.pt_window_expand(C.byref(cam), C.byref(win), -2, C.byref(out)) == -1
    for bad in ((40, 20, 40, 32), (40, 20, 101, 32), (-1, 0, 5, 5), (60, 20, 40, 32)):
        assert l.pt_window_expand(C.byref(cam), C.byref((C.c_int32 * 4)(*bad)), 0, C.byref(out)) == -1, bad


def test_bad_arguments_are_rejected_before_any_device_call():
    """A fake scene and fake device addresses: never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    base = 1 << 40
    scene, aov, prim, rays, tiles, frames, work = (C.c_void_p(base + (i << 24)) for i in range(7))
    off = lambda p, k: C.c_void_p(p.value + k)      # noqa: E731
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=PASSES)
    bc, bp = C.byref(cam), C.byref(prm)

    def params(**kw):
        return C.byref(ptamd.default_params(**{**dict(passes=PASSES), **kw}))

    window = [
        ("NULL scene", (None, bc, bp, 0, 0, 8, 8, aov, None)),
        ("NULL camera", (scene, None, bp, 0, 0, 8, 8, aov, None)),
        ("NULL params", (scene, bc, None, 0, 0, 8, 8, aov, None)),
        ("NULL aov", (scene, bc, bp, 0, 0, 8, 8, None, None)),
        ("aov + 8", (scene, bc, bp, 0, 0, 8, 8, off(aov, 8), None)),
        ("passes 0", (scene, bc, params(passes=0), 0, 0, 8, 8, aov, None)),
        ("first_pass -1", (scene, bc, params(first_pass=-1), 0, 0, 8, 8, aov, None)),
        ("seed limit", (scene, bc, params(first_pass=2 ** 31 // (W * H)), 0, 0, 8, 8, aov, None)),
        ("empty", (scene, bc, bp, 8, 8, 8, 16, aov, None)),
        ("inverted", (scene, bc, bp, 8, 8, 16, 4, aov, None)),
        ("x0 < 0", (scene, bc, bp, -1, 0, 8, 8, aov, None)),
        ("x1 > W", (scene, bc, bp, 0, 0, W + 1, 8, aov, None)),
        ("y1 > H", (scene, bc, bp, 0, 0, 8, H + 1, aov, None)),
        ("frame 1 x 5", (scene, C.byref(ptamd.make_camera(1, 5)), bp, 0, 0, 1, 1, aov, None)),
    ]
    for what, a in window:
        assert l.pt_render_aov_window(*a, None) == -1, what
    h_aov, h_prim = np.zeros((8, 8, 8), np.float32), np.zeros((8, 8), np.int32)
    P = ptamd._ptr
    for what, a in [("NULL scene", (None, bc, bp, 0, 0, 8, 8, P(h_aov), P(h_prim))), ("NULL aov", (scene, bc, bp, 0, 0, 8, 8, None, None)),
                    ("NULL camera", (scene, None, bp, 0, 0, 8, 8, P(h_aov), None)), ("x1 > W", (scene, bc, bp, 0, 0, W + 1, 8, P(h_aov), None)),
                    ("passes 0", (scene, bc, params(passes=0), 0, 0, 8, 8, P(h_aov), None))]:
        assert l.pt_aov_window(*a) == -1, what

    cams = (ptamd.PtCamera * 3)(cam, ptamd.make_camera(W, H, pos=(1, 20, 50)), ptamd.make_camera(W, H, fovy_deg=30.0))
    odd = (ptamd.PtCamera * 3)(cam, ptamd.make_camera(W, H + 1), cam)
    tiny = (ptamd.PtCamera * 1)(ptamd.make_camera(1, 5))
    huge = (ptamd.PtCamera * 17)(*[ptamd.make_camera(4096, 4096)] * 17)
    keep = [np.array([0, 5, 2], np.int32), np.array([0, -1, 2], np.int32), np.array([0, 0, 2 ** 31 // (W * H)], np.int32)]
    views = [
        ("NULL scene", (None, cams, 3, bp, None, aov, None)),
        ("NULL cameras", (scene, None, 3, bp, None, aov, None)),
        ("NULL params", (scene, cams, 3, None, None, aov, None)),
        ("NULL aov", (scene, cams, 3, bp, None, None, None)),
        ("aov + 4", (scene, cams, 3, bp, None, off(aov, 4), None)),
        ("n_views 0", (scene, cams, 0, bp, None, aov, None)),
        ("n_views -1", (scene, cams, -1, bp, None, aov, None)),
        ("unequal H", (scene, odd, 3, bp, None, aov, None)),
        ("frame 1 x 5", (scene, tiny, 1, bp, None, aov, None)),
        ("first_pass -1", (scene, cams, 3, bp, P(keep[1]), aov, None)),
        ("seed limit of view 2", (scene, cams, 3, bp, P(keep[2]), aov, None)),
        ("seed limit by prm", (scene, cams, 3, params(first_pass=2 ** 31 // (W * H)), None, aov, None)),
        ("passes 0", (scene, cams, 3, params(passes=0), P(keep[0]), aov, None)),
        ("2^28 pixels", (scene, huge, 17, params(passes=1), None, aov, None)),
    ]
    for what, a in views:
        assert l.pt_render_aov_views(*a, None) == -1, what
    h3 = np.zeros((3, H, W, 8), np.float32)
    for what, a in [("NULL scene", (None, cams, 3, bp, None, P(h3), None)), ("NULL aov", (scene, cams, 3, bp, None, None, None)),
                    ("unequal H", (scene, odd, 3, bp, None, P(h3), None)), ("first_pass -1", (scene, cams, 3, bp, P(keep[1]), P(h3), None))]:
        assert l.pt_aov_views(*a) == -1, what

    ray_cases = [
        ("NULL scene", (None, rays, 64, aov, prim)),
        ("NULL rays", (scene, None, 64, aov, prim)),
        ("NULL aov", (scene, rays, 64, None, prim)),
        ("n < 0", (scene, rays, -1, aov, prim)),
        ("rays + 4", (scene, off(rays, 4), 64, aov, None)),
        ("rays + 8", (scene, off(rays, 8), 64, aov, None)),
        ("aov + 8", (scene, rays, 64, off(aov, 8), None)),
        ("prim + 2", (scene, rays, 64, aov, off(prim, 2))),
        ("n = 0 does not excuse a NULL", (scene, None, 0, aov, None)),
    ]
    for what, a in ray_cases:
        assert l.pt_aov_rays(*a, None) == -1, what
        assert b"pt_aov_rays:" in l.pt_last_error(), (what, l.pt_last_error())
    h_rays, h8 = np.zeros((64, 8), np.float32), np.zeros((64, 8), np.float32)
    for what, a in [("NULL scene", (None, P(h_rays), 64, P(h8), None)), ("NULL rays", (scene, None, 64, P(h8), None)),
                    ("NULL aov", (scene, P(h_rays), 64, None, None)), ("n < 0", (scene, P(h_rays), -3, P(h8), None))]:
        assert l.pt_aov_rays_host(*a) == -1, what
    assert l.pt_aov_rays(scene, rays, 0, aov, None, None) == 0 and l.pt_aov_rays(scene, rays, 0, aov, prim, None) == 0      # nothing to do
    assert l.pt_aov_rays_host(scene, P(h_rays), 0, P(h8), None) == 0

    for what, a in [("NULL tiles", (None, bc, 3, frames)), ("NULL camera", (tiles, None, 3, frames)), ("NULL frames", (tiles, bc, 3, None)),
                    ("n_views 0", (tiles, bc, 0, frames)), ("frame 1 x 5", (tiles, C.byref(ptamd.make_camera(1, 5)), 3, frames)),
                    ("2^28 pixels", (tiles, C.byref(ptamd.make_camera(4096, 4096)), 17, frames))]:
        assert l.pt_untile_views(*a, None) == -1, what

    good = C.byref(ptamd.denoise_params())
    dn = lambda **kw: C.byref(ptamd.denoise_params(**kw))      # noqa: E731
    n = 3
    d_rgb, d_aov, d_out, d_work = tiles, aov, frames, work
    batch = [
        ("NULL rgb", (None, d_aov, 16, 8, n, 1, good, d_out, d_work)),
        ("NULL aov", (d_rgb, None, 16, 8, n, 1, good, d_out, d_work)),
        ("NULL params", (d_rgb, d_aov, 16, 8, n, 1, None, d_out, d_work)),
        ("NULL out", (d_rgb, d_aov, 16, 8, n, 1, good, None, d_work)),
        ("NULL work", (d_rgb, d_aov, 16, 8, n, 1, good, d_out, None)),
        ("W 1", (d_rgb, d_aov, 1, 8, n, 1, good, d_out, d_work)),
        ("H 1", (d_rgb, d_aov, 16, 1, n, 1, good, d_out, d_work)),
        ("n_frames 0", (d_rgb, d_aov, 16, 8, 0, 1, good, d_out, d_work)),
        ("n_frames -2", (d_rgb, d_aov, 16, 8, -2, 1, good, d_out, d_work)),
        ("n_frames 65536", (d_rgb, d_aov, 16, 8, 65536, 1, good, d_out, d_work)),
        ("2^28 pixels", (d_rgb, d_aov, 4096, 4096, 17, 1, good, d_out, d_work)),
        ("sample_cnt 0", (d_rgb, d_aov, 16, 8, n, 0, good, d_out, d_work)),
        ("iterations 13", (d_rgb, d_aov, 16, 8, n, 1, dn(iterations=13), d_out, d_work)),
        ("iterations -1", (d_rgb, d_aov, 16, 8, n, 1, dn(iterations=-1), d_out, d_work)),
        ("sigma 0", (d_rgb, d_aov, 16, 8, n, 1, dn(sigma_normal=0.0), d_out, d_work)),
        ("sigma nan", (d_rgb, d_aov, 16, 8, n, 1, dn(sigma_color=float("nan")), d_out, d_work)),
        ("aov + 4", (d_rgb, off(d_aov, 4), 16, 8, n, 1, good, d_out, d_work)),
        ("work + 8", (d_rgb, d_aov, 16, 8, n, 1, good, d_out, off(d_work, 8))),
        # the extents are those of n frames: an output that starts inside the third frame of the input overlaps it
        ("out inside rgb's third frame", (d_rgb, d_aov, 16, 8, n, 1, good, off(d_rgb, 16 * 8 * 12 * 2 + 16), d_work)),
        ("out inside the third frame's features", (d_rgb, d_aov, 16, 8, n, 1, good, off(d_aov, 16 * 8 * 32 * 2 + 64), d_work)),
        ("out inside the work buffer's last third", (d_rgb, d_aov, 16, 8, n, 1, good, off(d_work, 16 * 8 * 16 * n * 2 + 16 * 8 * 16 * 2), d_work)),
        ("work overlaps the features", (d_rgb, d_aov, 16, 8, n, 1, good, d_out, off(d_aov, 16 * 8 * 32 * 2))),
    ]
    for what, a in batch:
        assert l.pt_denoise_batch(*a, None) == -1, what
    rgb3, aov3, out3 = np.zeros((n, 8, 16, 3), np.float32), np.zeros((n, 8, 16, 8), np.float32), np.zeros((n, 8, 16, 3), np.float32)
    host = [
        ("NULL rgb", (0, None, P(aov3), 16, 8, n, 1, good, P(out3))),
        ("NULL aov", (0, P(rgb3), None, 16, 8, n, 1, good, P(out3))),
        ("NULL out", (0, P(rgb3), P(aov3), 16, 8, n, 1, good, None)),
        ("n_frames 0", (0, P(rgb3), P(aov3), 16, 8, 0, 1, good, P(out3))),
        ("n_frames 65536", (0, P(rgb3), P(aov3), 16, 8, 65536, 1, good, P(out3))),
        ("sample_cnt -1", (0, P(rgb3), P(aov3), 16, 8, n, -1, good, P(out3))),
        ("out is rgb", (0, P(rgb3), P(aov3), 16, 8, n, 1, good, P(rgb3))),
        ("out is rgb's last frame", (0, P(rgb3), P(aov3), 16, 8, n, 1, good, P(rgb3[2]))),
    ]
    for what, a in host:
        assert l.pt_denoise_batch_host(*a) == -1, what


def test_wrappers_check_shapes_on_the_host():
    class Fake:
        n_tris, device, _h = 5, 0, C.c_void_p(1 << 40)
    for bad in (np.zeros((4, 7), np.float32), np.zeros(8, np.float32), "rays"):
        with pytest.raises(ptamd.PtError):
            ptamd.Scene.aov_rays(Fake(), bad)
    with pytest.raises(ValueError):
        ptamd.denoise_batch(np.zeros((2, 4, 4, 3), np.float32), np.zeros((2, 4, 4, 7), np.float32), 1)
    with pytest.raises(ValueError):
        ptamd.denoise_batch(np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 8), np.float32), 1)
    with pytest.raises(ptamd.PtError):
        ptamd.Scene.aov_views(Fake(), [], ptamd.default_params())
    with pytest.raises(ptamd.PtError):
        ptamd.Scene.aov_views(Fake(), [ptamd.make_camera(W, H)] * 2, ptamd.default_params(), first_pass=[1, 2, 3])


def _cone_frame(seed):
    rs = np.random.RandomState(seed)
    aov = np.zeros((H, W, 8), np.float32)
    aov[..., 0:3] = rs.uniform(0.05, 1.0, (H, W, 3))
    n = rs.standard_normal((H, W, 3)) * 0.05 + (0.0, 0.0, 1.0)      # normals and depths that vary, but not enough to cut every tap off
    aov[..., 3:6] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    aov[..., 6] = rs.uniform(10.0, 10.5, (H, W))
    aov[..., 7] = 1.0
    rgb = rs.uniform(0.0, 4.0, (H, W, 3)).astype(np.float32)
    rgb[25, 45] = np.nan
    rgb[0, 0] = np.nan
    rgb[3, 17, 1] = np.inf
    rgb[30, 58, 2] = -np.inf
    rgb[8:14, 6:12] = np.nan              # a block whose centre outlives the first iteration
    rgb[22:27, 50:55, 0] = np.nan
    return rgb, aov


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("win", DN_WINDOWS)
def test_cone_of_the_definition(L, win):
    """denoise_ref.denoise of the window grown by M = 2 (2^L - 1), cropped, is the crop of the full frame's: to 1e-12 relative (numpy's
    vector exp need not give the same bits at different array offsets; bit equality is asserted on the GPU, where both sides are the
    same kernel) and with the same non-finite positions."""
    rgb, aov = _cone_frame(11)
    kw = dict(D.DEFAULTS, iterations=L)
    M = ptamd.denoise_margin(L)
    ex = expand(win, M, W, H)
    assert ex == ptamd.expand_window(ptamd.make_camera(W, H), win, M)
    full = crop(D.denoise(rgb, aov, 3, **kw), win)
    part = crop(D.denoise(crop(rgb, ex), crop(aov, ex), 3, **kw), win, ex[:2])
    assert full.shape == part.shape == (win[3] - win[1], win[2] - win[0], 3)
    assert np.array_equal(np.isfinite(full), np.isfinite(part)) and np.array_equal(np.isnan(full), np.isnan(part))
    m = np.isfinite(full)
    assert m.mean() > 0.5
    assert (np.abs(full[m] - part[m]) <= 1e-12 * np.abs(full[m])).all(), float((np.abs(full[m] - part[m]) / np.abs(full[m])).max())
    assert np.nanmax(np.abs(full[m] - crop(rgb, win).astype(np.float64)[m])) > 1e-3      # the filter did something


def test_cone_margin_is_the_bound_and_not_slack():
    """L = 3, M = 14, window (40, 20, 60, 32): column 26 reaches column 40 by the taps 26 -> 28 (step 1), 28 -> 32 (step 2), 32 -> 40
    (step 4).  A frame that is flat but for a bright column 26: with margin M the crop is the full frame's, with M - 1 (column 26 dropped)
    it is not."""
    L, win = 3, DN_WINDOWS[0]
    M = ptamd.denoise_margin(L)
    assert M == 14 and win[0] - M == 26
    rgb = np.full((H, W, 3), 1.0, np.float32)
    rgb[:, 26] = 50.0
    aov = np.zeros((H, W, 8), np.float32)
    aov[..., 0:3] = 0.5
    aov[..., 5] = 1.0
    aov[..., 6] = 10.0
    aov[..., 7] = 1.0
    kw = dict(D.DEFAULTS, iterations=L, sigma_color=1e4)
    full = crop(D.denoise(rgb, aov, 1, **kw), win)
    out = {}
    for m in (M, M - 1):
        ex = expand(win, m, W, H)
        out[m] = crop(D.denoise(crop(rgb, ex), crop(aov, ex), 1, **kw), win, ex[:2])
    assert (np.abs(out[M] - full) <= 1e-12 * np.abs(full)).all()
    d = np.abs(out[M - 1] - full) / np.abs(full)
    print(f"margin M - 1: column 40 of the window differs by {d[:, 0].max():.3e} relative, the other columns by at most {d[:, 1:].max():.3e}")
    assert d[:, 0].min() > 1e-6 and d[:, 1:].max() <= 1e-12      # exactly the column whose cone touches column 26


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _build(name):
    def make():
        prims = ptamd.gen_scene(0) if name == "cornell" else ptamd.gen_scene(1, 16)
        nodes, tris, _ = ptamd.build_bvh(prims)
        return nodes, tris, (make_test_spheres() if name == "standin_spheres" else None)
    return _cached(("build", name), make)


def _scene(name):
    return _cached(("scene", name), lambda: ptamd.Scene(*_build(name)))


def _params(**kw):
    return ptamd.default_params(**{**dict(passes=PASSES, first_pass=3), **kw})


def _full_aov(name, cam_key, cam, **kw):
    """Scene.aov of the full frame, computed once per (scene, camera, params) and never written to."""
    def make():
        a, p = _scene(name).aov(cam, _params(**kw))
        a.setflags(write=False)
        p.setflags(write=False)
        return a, p
    return _cached(("aov", name, cam_key, tuple(sorted(kw.items()))), make)


VIEW_CAMERAS = [dict(), dict(pos=(6.0, 24.0, 52.0), rot_deg=(0.0, 80.0, 5.0), fovy_deg=60.0), dict(pos=(-10.0, 12.0, 45.0), rot_deg=(8.0, 100.0, 0.0), fovy_deg=30.0)]
VIEW_FIRST = [0, 5, 2]


def _view_cams(w=W, h=H):
    return [ptamd.make_camera(w, h, **kw) for kw in VIEW_CAMERAS]


@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    O.set_libm(1)
    yield


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "standin_spheres"])
def test_window_aov_is_the_crop_of_the_full_frames(_gpu, name):
    sc, cam = _scene(name), ptamd.make_camera(W, H)
    assert 3 * sc.tree_info()["quad_depth"] + 2 <= 40      # the 4-wide walk
    full, fprim = _full_aov(name, "cam0", cam)
    assert (fprim >= 0).mean() > 0.5 and (name == "cornell" or (fprim >= sc.n_tris).any())      # the sphere pass is seen
    for win in WINDOWS:
        got, prim = sc.aov_window(cam, _params(), win)
        assert got.shape == (win[3] - win[1], win[2] - win[0], 8)
        assert same(got, crop(full, win)), (name, win)
        assert np.array_equal(prim, crop(fprim, win)), (name, win)
    # only passes and first_pass are read, as in pt_render_aov
    got, prim = sc.aov_window(cam, _params(rank=1, world=3, spp_per_pass=7, max_bounce=2), WINDOWS[1])
    assert same(got, crop(full, WINDOWS[1])) and np.array_equal(prim, crop(fprim, WINDOWS[1]))
    if name == "standin_spheres":
        nodes, tris, sph = _build(name)
        want, wprim = D.aov_from_oracle(O.Scene(nodes.tobytes(), tris, sph), O.make_camera(W, H), W, H, PASSES, 3)
        got, prim = sc.aov_window(cam, _params(), WINDOWS[1])
        assert same(got, crop(want, WINDOWS[1])) and np.array_equal(prim, crop(wprim, WINDOWS[1]))


@pytest.mark.gpu
def test_window_aov_on_device_pointers_writes_the_window_and_nothing_else(_gpu):
    import torch
    sc, cam, win = _scene("standin_spheres"), ptamd.make_camera(W, H), WINDOWS[1]
    full, fprim = _full_aov("standin_spheres", "cam0", cam)
    dev = torch.device("cuda:0")
    n = (win[3] - win[1]) * (win[2] - win[0])
    buf = torch.full((n * 8 + 64,), -7.0, dtype=torch.float32, device=dev)
    pbuf = torch.full((n + 16,), -9, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    sc.render_aov_window(cam, _params(), win, buf.data_ptr(), pbuf.data_ptr(), st.cuda_stream)
    sc.render_aov_window(cam, _params(), win, buf.data_ptr(), 0, st.cuda_stream)      # d_prim may be NULL
    st.synchronize()
    h, hp = buf.cpu().numpy(), pbuf.cpu().numpy()
    assert same(h[:n * 8].reshape(win[3] - win[1], win[2] - win[0], 8), crop(full, win)) and (h[n * 8:] == -7.0).all()
    assert np.array_equal(hp[:n].reshape(win[3] - win[1], win[2] - win[0]), crop(fprim, win)) and (hp[n:] == -9).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "standin_spheres"])
def test_view_aovs_are_each_cameras_own(_gpu, name):
    sc, cams = _scene(name), _view_cams()
    assert ((W + 7) // 8) * ((H + 7) // 8) == 91      # tile -> view is no power-of-two split
    got, prim = sc.aov_views(cams, _params(first_pass=9), VIEW_FIRST)
    assert got.shape == (3, H, W, 8) and prim.shape == (3, H, W)
    for v, cam in enumerate(cams):
        want, wprim = _full_aov(name, f"view{v}", cam, first_pass=VIEW_FIRST[v])
        assert same(got[v], want) and np.array_equal(prim[v], wprim), (name, v)
    assert not same(got[0], got[1]) and not same(got[1], got[2])
    got, prim = sc.aov_views(cams, _params())      # h_first_pass = NULL: prm.first_pass for every view
    for v, cam in enumerate(cams):
        want, wprim = _full_aov(name, f"view{v}", cam)
        assert same(got[v], want) and np.array_equal(prim[v], wprim), (name, v)
    one, p1 = sc.aov_views(cams[1:2], _params(), [5])
    assert same(one[0], _full_aov(name, "view1", cams[1], first_pass=5)[0])


def _repack(t, prim, surf):
    """The feature record of a ray from the 29-float record of trace_rays(surface=True): (0 + x) / 1 of fields 20..22, 8..10 and 1,
    coverage 1; zeros for a miss."""
    out = np.zeros((len(t), 8), np.float32)
    hit = prim >= 0
    with np.errstate(invalid="ignore"):
        x = np.concatenate([surf[:, 20:23], surf[:, 8:11], surf[:, 1:2]], 1).astype(np.float32)
        out[hit, :7] = ((np.float32(0) + x) / np.float32(1))[hit]
    out[hit, 7] = 1.0
    return out


def _mixed_rays(n):
    """scene_rays8 (axis-aligned, unnormalised and shortened rays among them) alternating with pinhole rays; every 7th ray cut short of
    anything (tmax 1e-3), every 11th sent out through the open front of the room."""
    a = scene_rays8(n, np.random.RandomState(7))
    b = pinhole_rays(ptamd.make_camera(64, 48))
    rays = a.copy()
    rays[1::2] = b[np.linspace(0, len(b) - 1, len(rays[1::2])).astype(int)]
    rays[6::7, 7] = 1e-3
    rays[10::11, 0:3] = (0.0, 20.0, 60.0)
    rays[10::11, 3:6] = (0.0, 0.0, 1.0)
    return np.ascontiguousarray(rays, np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "standin_spheres"])
@pytest.mark.parametrize("n", [1, 130, 64 * 48])
def test_ray_aovs_are_the_repack_of_the_closest_hit_query(_gpu, name, n):
    sc = _scene(name)
    rays = _mixed_rays(max(n, 2))[:n] if n > 1 else _mixed_rays(8)[4:5]
    t, prim, surf = sc.trace_rays(rays, surface=True)
    got, gprim = sc.aov_rays(rays)
    assert got.shape == (n, 8) and np.array_equal(gprim, prim)
    assert same(got, _repack(t, prim, surf)), (name, n)
    assert (got[prim < 0] == 0).all() and (bits(got[prim < 0]) == 0).all() and (got[prim >= 0, 7] == 1).all()
    if n > 100:
        assert (prim < 0).any() and (prim >= 0).mean() > 0.3


@pytest.mark.gpu
def test_ray_aovs_of_a_cameras_rays_are_one_pass_of_its_aov(_gpu):
    import torch
    sc, cam = _scene("standin_spheres"), ptamd.make_camera(64, 48)
    rays, _, _ = ptamd.camera_rays(cam, 4)
    want, wprim = sc.aov(cam, ptamd.default_params(passes=1, first_pass=4))
    got, prim = sc.aov_rays(rays)
    assert same(got.reshape(48, 64, 8), want) and np.array_equal(prim.reshape(48, 64), wprim)
    # the device path on a stream, in place, without the primitive buffer
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        d_rays = torch.from_numpy(rays).to(dev)
        d_got, d_prim = sc.aov_rays(d_rays, stream_ptr=st.cuda_stream)
        d_only = torch.empty_like(d_got)
        sc.aov_rays_device(d_rays.data_ptr(), len(rays), d_only.data_ptr(), 0, st.cuda_stream)
    st.synchronize()
    assert same(d_got.cpu().numpy(), got) and np.array_equal(d_prim.cpu().numpy(), prim) and same(d_only.cpu().numpy(), got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain28", "comb32"])
def test_binary_walk_on_trees_past_the_cut(_gpu, name):
    """4-wide depth 13 (the first past the cut at 12) and binary depth 32: 3 * quad_depth + 2 > 40, so the kernel walks the binary tree
    with trace_closest, as pt_trace_rays does."""
    sc = T.device_scene(name)
    info = sc.tree_info()
    assert 3 * info["quad_depth"] + 2 > 40 and (info["depth"], info["quad_depth"]) == T.TREES[name][2]
    cam, ocam = T.camera_of(name), T.camera_of(name, O)
    want, wprim = _cached(("oracle_aov", name, 3), lambda: D.aov_from_oracle(T.oracle_scene(name), ocam, T.W, T.H, PASSES, 3))
    assert (wprim >= 0).mean() > 0.1
    full, fprim = sc.aov(cam, _params())
    assert same(full, want) and np.array_equal(fprim, wprim)
    for win in ((0, 0, T.W, T.H), (3, 5, 37, 29), (57, 41, 64, 48)):
        got, prim = sc.aov_window(cam, _params(), win)
        assert same(got, crop(want, win)) and np.array_equal(prim, crop(wprim, win)), (name, win)
    want0, wprim0 = _cached(("oracle_aov", name, 0), lambda: D.aov_from_oracle(T.oracle_scene(name), ocam, T.W, T.H, PASSES, 0))
    got, prim = sc.aov_views([cam, cam], _params(), [3, 0])
    assert same(got[0], want) and np.array_equal(prim[0], wprim) and same(got[1], want0) and np.array_equal(prim[1], wprim0)
    rays = T.query_rays(name)
    t, qprim, surf = sc.trace_rays(rays, surface=True)
    got, prim = sc.aov_rays(rays)
    assert np.array_equal(prim, qprim) and same(got, _repack(t, qprim, surf))
    assert (qprim >= 0).sum() >= 64 and (qprim < 0).sum() >= 64      # hits and misses, more than a wave of each (the chain is a small target)


@pytest.mark.gpu
def test_window_aov_after_an_update_and_a_rebuild_on_the_same_stream(_gpu):
    import torch
    nodes, tris, sph = _build("standin_spheres")
    sc, cam, win = ptamd.Scene(nodes, tris, sph), ptamd.make_camera(W, H), (3, 5, 99, 50)
    before, _ = sc.aov_window(cam, _params(), win)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    n = (win[3] - win[1]) * (win[2] - win[0])
    with torch.cuda.stream(st):
        pos = torch.from_numpy(R.positions(tris)).to(dev)
        sel = torch.from_numpy(R.mesh_mask(tris)).to(dev)
        d_pos = R.move_rigid_wobble(pos, sel, torch).reshape(-1, 9).contiguous()
        d_aov = torch.empty(n * 8, dtype=torch.float32, device=dev)
        d_prim = torch.empty(n, dtype=torch.int32, device=dev)
        sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
        sc.rebuild_tree(st.cuda_stream)
        sc.render_aov_window(cam, _params(), win, d_aov.data_ptr(), d_prim.data_ptr(), st.cuda_stream)      # no host wait of ours in between
        got, gprim = d_aov.cpu().numpy().reshape(win[3] - win[1], win[2] - win[0], 8), d_prim.cpu().numpy().reshape(win[3] - win[1], win[2] - win[0])
        h_pos = d_pos.cpu().numpy()
    st.synchronize()
    tris2 = R.restate_tris(tris, h_pos)
    fresh = ptamd.Scene(R.refit_nodes(nodes, tris2), tris2, sph)
    want, wprim = fresh.aov(cam, _params())
    assert same(got, crop(want, win)) and np.array_equal(gprim, crop(wprim, win))
    moved = (bits(got) != bits(before)).any(-1).mean()
    print(f"the move changed {moved:.4f} of the window's pixels")
    assert moved > 0.02


def _batch_frames():
    """Three rendered 64 x 48 views with their feature buffers, NaN and +-inf pixels injected; computed once."""
    def make():
        sc, cams = _scene("standin_spheres"), _view_cams(64, 48)
        prm = ptamd.default_params(passes=PASSES, spp_per_pass=2)
        rgb = sc.render_views(cams, prm)
        aov, _ = sc.aov_views(cams, prm)
        rgb[0, 10, 10] = np.nan
        rgb[0, 0, 0] = np.nan
        rgb[1, 47, 63, 0] = np.nan
        rgb[1, 20, 30, 1] = np.inf
        rgb[2, 30, 50, 2] = -np.inf
        rgb[2, 0, 5:11] = np.nan                    # first rows of frame 2: the taps above them belong to frame 1 in the stack
        rgb[1, 42:48, 20:26] = np.nan               # last rows of frame 1, a block
        rgb.setflags(write=False)
        aov.setflags(write=False)
        return rgb, aov
    return _cached("batch_frames", make)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [0, 1, 5])
def test_denoise_batch_is_denoise_of_every_slice(_gpu, L):
    rgb, aov = _batch_frames()
    got = ptamd.denoise_batch(rgb, aov, PASSES, iterations=L)
    for k in range(3):
        assert same(got[k], ptamd.denoise(rgb[k], aov[k], PASSES, iterations=L)), (L, k)
    if L == 0:
        assert np.array_equal(bits(got), bits(rgb))      # one copy, NaN bits included
    else:
        assert not same(got, rgb)


@pytest.mark.gpu
def test_denoise_batch_taps_do_not_cross_frames(_gpu):
    rgb, aov = _batch_frames()
    got = ptamd.denoise_batch(rgb, aov, PASSES)
    order = [2, 0, 1]
    again = ptamd.denoise_batch(rgb[order], aov[order], PASSES)
    for k, src in enumerate(order):
        assert same(again[k], got[src]), (k, src)
    alone = ptamd.denoise_batch(rgb[1:2], aov[1:2], PASSES, sigma_color=4.0, demodulate=0)
    assert same(alone[0], ptamd.denoise(rgb[1], aov[1], PASSES, sigma_color=4.0, demodulate=0))


@pytest.mark.gpu
def test_untile_views_is_untile_per_view_and_the_batch_runs_on_device_pointers(_gpu):
    import torch
    sc, cams = _scene("standin_spheres"), _view_cams()
    prm = ptamd.default_params(passes=PASSES, spp_per_pass=2)
    V = len(cams)
    dev = torch.device("cuda:0")
    tiles = torch.empty(ptamd.views_floats(cams[0], V), dtype=torch.float32, device=dev)
    work = torch.empty(max(ptamd.views_work_bytes(cams[0], prm, V), ptamd.denoise_batch_work_bytes(W, H, V)), dtype=torch.uint8, device=dev)
    frames = torch.full((V, H, W, 3), -1.0, dtype=torch.float32, device=dev)
    each = torch.full((V, H, W, 3), -2.0, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    sc.render_views_device(cams, prm, tiles.data_ptr(), work.data_ptr(), st)
    ptamd.untile_views(tiles.data_ptr(), cams[0], V, frames.data_ptr(), st)
    T_ = tiles.numel() // V
    for v in range(V):
        ptamd.untile(tiles[v * T_:].data_ptr(), cams[v], 1, each[v].data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.equal(frames.view(torch.int32), each.view(torch.int32))
    assert same(frames.cpu().numpy(), sc.render_views(cams, prm))
    # the stacked frames straight into the batch, on the device
    aov = torch.empty((V, H, W, 8), dtype=torch.float32, device=dev)
    out = torch.empty_like(frames)
    sc.render_aov_views(cams, prm, aov.data_ptr(), 0, st)
    ptamd.denoise_batch_device(frames.data_ptr(), aov.data_ptr(), W, H, V, PASSES, out.data_ptr(), work.data_ptr(), st, iterations=2)
    torch.cuda.synchronize()
    h_rgb, h_aov, h_out = frames.cpu().numpy(), aov.cpu().numpy(), out.cpu().numpy()
    for v in range(V):
        assert same(h_out[v], ptamd.denoise(h_rgb[v], h_aov[v], PASSES, iterations=2)), v


@pytest.mark.gpu
def test_windowed_denoise_is_the_crop_of_the_full_frames(_gpu):
    sc, cam = _scene("standin_spheres"), ptamd.make_camera(W, H)
    prm = ptamd.default_params(passes=PASSES, spp_per_pass=2)
    rgb = sc.render(cam, prm)
    aov, _ = sc.aov(cam, prm)
    for kw in (dict(iterations=3), dict()):      # L = 3 with its own margin 14; the default L = 5, margin 62
        full = ptamd.denoise(rgb, aov, PASSES, **kw)
        for win in DN_WINDOWS:
            got = sc.render_window_denoised(cam, prm, win, **kw)
            assert got.shape == (win[3] - win[1], win[2] - win[0], 3)
            assert same(got, crop(full, win)), (kw, win)
    # a margin of 0 is defined as the denoise of the window itself, with no equality claim
    win = DN_WINDOWS[0]
    got = sc.render_window_denoised(cam, prm, win, margin=0, iterations=3)
    assert same(got, ptamd.denoise(crop(rgb, win), crop(aov, win), PASSES, iterations=3))
    assert not same(got, crop(ptamd.denoise(rgb, aov, PASSES, iterations=3), win))


@pytest.mark.gpu
def test_views_denoised_is_render_aov_denoise_per_view(_gpu):
    sc, cams = _scene("standin_spheres"), _view_cams()
    prm = ptamd.default_params(passes=PASSES, spp_per_pass=2)
    got = sc.render_views_denoised(cams, prm, VIEW_FIRST, iterations=3)
    assert got.shape == (3, H, W, 3)
    for v, cam in enumerate(cams):
        p = ptamd.default_params(passes=PASSES, spp_per_pass=2, first_pass=VIEW_FIRST[v])
        want = ptamd.denoise(sc.render(cam, p), sc.aov(cam, p)[0], PASSES, iterations=3)
        assert same(got[v], want), v


@pytest.mark.gpu
def test_new_calls_have_no_side_effects(_gpu):
    nodes, tris, sph = _build("standin_spheres")
    sc, cam, cams = ptamd.Scene(nodes, tris, sph), ptamd.make_camera(W, H), _view_cams()
    prm = ptamd.default_params(passes=PASSES, spp_per_pass=4)
    before = sc.render(cam, prm)
    frame_aov = sc.aov(cam, prm)
    iters, dbytes = sc.last_iterations(), sc.device_bytes
    sc.aov_window(cam, prm, WINDOWS[1])
    sc.aov_rays(_mixed_rays(130))
    assert (sc.last_iterations(), sc.device_bytes) == (iters, dbytes)
    sc.aov_views(cams, prm, VIEW_FIRST)      # may grow the scene's view table, which pt_scene_device_bytes does not count
    ptamd.denoise_batch(np.stack([before] * 2), np.stack([frame_aov[0]] * 2), PASSES, iterations=2)
    assert (sc.last_iterations(), sc.device_bytes) == (iters, dbytes)
    after = sc.render(cam, prm)
    assert np.array_equal(bits(after), bits(before)) and sc.last_iterations() == iters
    again = sc.aov(cam, prm)
    assert same(again[0], frame_aov[0]) and np.array_equal(again[1], frame_aov[1])
    # a batch of views rendered after the feature buffers used the same table
    assert same(sc.render_views(cams[:2], prm)[0], before)
