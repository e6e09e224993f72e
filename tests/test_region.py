"""A pixel window or any list of tiles without the full frame (pt_render_tile_list, pt_tile_list_floats, pt_tile_list_work_bytes,
pt_tiles_of_window, pt_untile_list, pt_render_window, ptrender --window): the C-ABI surface, the window-to-tiles rule and the
argument checks on the CPU; on the GPU equality of bits with the full-frame render (windows, list order, per-pass means, the
scatter, side effects, the CLI) and the CPU oracle's own window render as the check that is not the code under test."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import ptamd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pt_render_tile_list", "pt_tile_list_floats", "pt_tile_list_work_bytes", "pt_tiles_of_window", "pt_untile_list",
               "pt_render_window")
SCENES = {"cornell": (0, 187), "standin": (1, 24)}
FRAMES = ((64, 48), (100, 52))      # whole tiles, and ragged on both edges
PASSES, FIRST_PASS, SPP = 3, 2, 4
REL_RMS_TOL = 1e-4                  # north_star tolerance (tests/test_gpu_parity.py)
PATTERN = 0x7FC12345                # a NaN payload no render produces


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits_or_nan(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def windows(W, H):
    """aligned | unaligned | one pixel | one pixel in the last (ragged) tile | touching the right and bottom edges | whole frame"""
    return ((8, 8, 32, 24), (5, 3, 37, 29), (W // 2, H // 2, W // 2 + 1, H // 2 + 1), (W - 1, H - 1, W, H), (W - 13, H - 9, W, H),
            (0, 0, W, H))


def tiles_of_window_ref(W, win):
    x0, y0, x1, y1 = win
    tx, ty = np.arange(x0 // 8, (x1 - 1) // 8 + 1), np.arange(y0 // 8, (y1 - 1) // 8 + 1)
    return (ty[:, None] * ((W + 7) // 8) + tx[None, :]).ravel().astype(np.int32)


def n_tiles_of(W, H):
    return ((W + 7) // 8) * ((H + 7) // 8)


def params(**kw):
    return ptamd.default_params(**{**dict(passes=PASSES, first_pass=FIRST_PASS, spp_per_pass=SPP), **kw})


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: C-ABI surface, the window rule, argument checks, the size of the work buffer (no device is touched)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound():
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in NEW_SYMBOLS:
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    for name in ("render_tile_list", "render_window", "render_tile_list_device"):
        assert callable(getattr(ptamd.Scene, name))
    for name in ("tiles_of_window", "untile_list", "tile_list_floats", "tile_list_work_bytes"):
        assert callable(getattr(ptamd, name))
    assert ptamd.tile_list_floats(1) == 192 and ptamd.tile_list_floats(48) == 48 * 192
    assert ptamd.lib().pt_tile_list_floats(0) == -1 and ptamd.lib().pt_tile_list_floats(-3) == -1


def test_tiles_of_window_matches_its_restatement():
    l = ptamd.lib()
    for W, H in FRAMES:
        cam = ptamd.make_camera(W, H)
        for win in windows(W, H):
            want = tiles_of_window_ref(W, win)
            got = ptamd.tiles_of_window(cam, win)
            assert got.dtype == np.int32 and np.array_equal(got, want), (W, H, win)
            assert np.all(np.diff(got) > 0) or got.size == 1
            # the count without a buffer, and a buffer that is too small is filled up to its size only
            assert l.pt_tiles_of_window(C.byref(cam), *win, None, 0) == want.size
            buf = np.full(want.size + 2, -7, np.int32)
            cap = max(want.size - 1, 0)
            assert l.pt_tiles_of_window(C.byref(cam), *win, ptamd._ptr(buf), cap) == want.size
            assert np.array_equal(buf[:cap], want[:cap]) and (buf[cap:] == -7).all()
        assert ptamd.tiles_of_window(cam, (0, 0, W, H)).size == n_tiles_of(W, H)
        for bad in ((8, 8, 8, 16), (8, 8, 16, 8), (16, 8, 8, 16), (8, 16, 16, 8), (-1, 0, 8, 8), (0, -8, 8, 8), (0, 0, W + 1, 8),
                    (0, 0, 8, H + 1), (W, 0, W + 8, 8), (W + 8, H + 8, W + 16, H + 16)):
            assert l.pt_tiles_of_window(C.byref(cam), *bad, None, 0) == -1, (W, H, bad)
            with pytest.raises(ptamd.PtError):
                ptamd.tiles_of_window(cam, bad)
    assert l.pt_tiles_of_window(None, 0, 0, 8, 8, None, 0) == -1
    assert l.pt_tiles_of_window(C.byref(ptamd.make_camera(64, 48)), 0, 0, 8, 8, None, 4) == -1      # cap without a buffer


def test_bad_arguments_are_rejected_before_any_device_call():
    """Fake device addresses and a fake scene: they are never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    W, H = 100, 52
    cam, prm = ptamd.make_camera(W, H), params()
    bc, bp = C.byref(cam), C.byref(prm)
    base = 1 << 40
    scene, d_tiles, d_work, d_out = (C.c_void_p(base + (i << 20)) for i in range(4))
    n_total = n_tiles_of(W, H)
    ok = np.array([3, 0, 90], np.int32)
    lst = lambda a: ptamd._ptr(np.ascontiguousarray(a, np.int32))      # noqa: E731
    render = [
        (None, bc, bp, lst(ok), 3, d_tiles, d_work),
        (scene, None, bp, lst(ok), 3, d_tiles, d_work),
        (scene, bc, None, lst(ok), 3, d_tiles, d_work),
        (scene, bc, bp, None, 3, d_tiles, d_work),
        (scene, bc, bp, lst(ok), 3, None, d_work),
        (scene, bc, bp, lst(ok), 3, d_tiles, None),
        (scene, bc, bp, lst(ok), 0, d_tiles, d_work),
        (scene, bc, bp, lst(ok), -2, d_tiles, d_work),
        (scene, bc, bp, lst(np.arange(n_total + 1)), n_total + 1, d_tiles, d_work),
        (scene, bc, bp, lst([3, n_total, 5]), 3, d_tiles, d_work),                      # out of range
        (scene, bc, bp, lst([3, -1, 5]), 3, d_tiles, d_work),
        (scene, bc, bp, lst([3, 5, 3]), 3, d_tiles, d_work),                            # twice
        (scene, bc, C.byref(params(rank=0, world=2)), lst(ok), 3, d_tiles, d_work),
        (scene, bc, C.byref(params(rank=1, world=2)), lst(ok), 3, d_tiles, d_work),
        (scene, bc, C.byref(params(passes=0)), lst(ok), 3, d_tiles, d_work),
        (scene, C.byref(ptamd.make_camera(1, 8)), bp, lst([0]), 1, d_tiles, d_work),
    ]
    for i, a in enumerate(render):
        assert l.pt_render_tile_list(*a, None) == -1, i
    l.pt_render_tile_list(*render[11], None)
    assert "twice" in l.pt_last_error().decode()
    win = (8, 8, 40, 24)
    untile = [
        (None, lst(ok), 3, bc, *win, d_out),
        (d_tiles, None, 3, bc, *win, d_out),
        (d_tiles, lst(ok), 3, None, *win, d_out),
        (d_tiles, lst(ok), 3, bc, *win, None),
        (d_tiles, lst(ok), 0, bc, *win, d_out),
        (d_tiles, lst([3, n_total]), 2, bc, *win, d_out),
        (d_tiles, lst([-4]), 1, bc, *win, d_out),
        (d_tiles, lst(ok), 3, bc, 8, 8, 8, 24, d_out),                                  # empty
        (d_tiles, lst(ok), 3, bc, 40, 8, 8, 24, d_out),                                 # inverted
        (d_tiles, lst(ok), 3, bc, 8, 8, W + 1, 24, d_out),                              # outside the frame
        (d_tiles, lst(ok), 3, bc, 8, -1, 40, 24, d_out),
    ]
    for i, a in enumerate(untile):
        assert l.pt_untile_list(*a, None) == -1, i
    rgb = np.zeros((16, 32, 3), np.float32)
    window = [
        (None, bc, bp, *win, ptamd._ptr(rgb)),
        (scene, None, bp, *win, ptamd._ptr(rgb)),
        (scene, bc, None, *win, ptamd._ptr(rgb)),
        (scene, bc, bp, *win, None),
        (scene, bc, bp, 8, 8, 8, 24, ptamd._ptr(rgb)),
        (scene, bc, bp, 40, 24, 8, 8, ptamd._ptr(rgb)),
        (scene, bc, bp, 8, 8, W + 1, 24, ptamd._ptr(rgb)),
        (scene, bc, bp, W, H, W + 8, H + 8, ptamd._ptr(rgb)),
        (scene, bc, bp, -8, 8, 40, 24, ptamd._ptr(rgb)),
        (scene, bc, C.byref(params(spp_per_pass=0)), *win, ptamd._ptr(rgb)),
    ]
    for i, a in enumerate(window):
        assert l.pt_render_window(*a) == -1, i
    for a in ((None, bp, 1), (bc, None, 1), (bc, bp, 0), (bc, bp, n_total + 1), (bc, C.byref(params(rank=1, world=2)), 1)):
        assert l.pt_tile_list_work_bytes(*a) == -1, a
    with pytest.raises(ptamd.PtError):
        ptamd.tile_list_work_bytes(cam, prm, 0)


def test_work_bytes_are_those_of_a_frame_with_as_many_tiles():
    prm = ptamd.default_params(passes=8)
    cam = ptamd.make_camera(1920, 1080)
    for n in (1, 6, 48):
        assert ptamd.tile_list_work_bytes(cam, prm, n) == ptamd.work_bytes(ptamd.make_camera(8 * n, 8), prm), n
    assert ptamd.tile_list_work_bytes(cam, prm, 1) < ptamd.work_bytes(cam, prm) // 50
    for W, H in FRAMES:
        c = ptamd.make_camera(W, H)
        assert ptamd.tile_list_work_bytes(c, prm, n_tiles_of(W, H)) == ptamd.work_bytes(c, prm), (W, H)


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


def _prims(name):
    kind, lat_lon = SCENES[name]
    return ptamd.gen_scene(kind, lat_lon)


def _scene(name):
    return ptamd.Scene.from_prims(_prims(name))


def _check_image(img_g, img_o, what):
    """The criterion of tests/test_gpu_parity.py, restated."""
    a, b = np.asarray(img_g, np.float64), np.asarray(img_o, np.float64)
    rr = float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))
    same = (bits(img_g) == bits(img_o)).all(-1)
    print(f"{what}: relRMS {rr:.3e}, bit-identical pixels {same.mean():.6f}")
    assert np.isfinite(img_g).all()
    assert rr <= REL_RMS_TOL, f"{what}: relative RMS {rr:.3e} > {REL_RMS_TOL}"
    assert same.mean() >= 0.999, f"{what}: only {same.mean():.5f} of pixels bit-identical"


def _check_against_oracle(img_g, so, W, H, win, prm, what, nthreads=16):
    import oracle_lib as O
    x0, y0, x1, y1 = win
    op = O.make_params(W, H, prm.passes, prm.spp_per_pass, first_pass=prm.first_pass, window=win)
    ref = so.render(O.make_camera(W, H), op, nthreads)[0][y0:y1, x0:x1]
    assert img_g.shape == ref.shape
    if np.isfinite(ref).all():
        _check_image(img_g, ref, what)
    else:      # one of the reference's own NaN pixels: the same bits, NaN where it has NaN
        assert same_bits_or_nan(img_g, ref).all(), what


class Device:
    """torch buffers for the device-pointer calls of one (scene, camera); everything on one stream."""

    def __init__(self, sc, cam):
        import torch
        self.torch, self.sc, self.cam = torch, sc, cam
        self.dev = torch.device("cuda:0")
        self.stream = torch.cuda.Stream(self.dev)
        self.n_total = n_tiles_of(cam.W, cam.H)

    def full(self, prm):
        """pt_render_tiles(world 1): (tiles (n_total, 192), per-pass means (passes, n_total, 192)) as numpy."""
        t = self.torch
        n = ptamd.tiles_floats(self.cam, prm)
        tiles = t.empty(n, dtype=t.float32, device=self.dev)
        work = t.empty(ptamd.work_bytes(self.cam, prm), dtype=t.uint8, device=self.dev)
        self.sc.render_tiles(self.cam, prm, tiles.data_ptr(), work.data_ptr(), self.stream.cuda_stream)
        with t.cuda.stream(self.stream):
            slab = work[:prm.passes * n * 4].view(t.float32).cpu().numpy().reshape(prm.passes, self.n_total, 192)
            out = tiles.cpu().numpy().reshape(self.n_total, 192)
        self.stream.synchronize()
        return out, slab

    def listed(self, prm, tiles, keep=False):
        """pt_render_tile_list with a work buffer of exactly pt_tile_list_work_bytes: (tiles (n, 192), per-pass means (passes, n, 192))."""
        t = self.torch
        tiles = np.ascontiguousarray(tiles, np.int32)
        n = tiles.size
        buf = t.empty(ptamd.tile_list_floats(n), dtype=t.float32, device=self.dev)
        work = t.empty(ptamd.tile_list_work_bytes(self.cam, prm, n), dtype=t.uint8, device=self.dev)
        self.sc.render_tile_list_device(self.cam, prm, tiles, buf.data_ptr(), work.data_ptr(), self.stream.cuda_stream)
        if keep:
            return buf
        with t.cuda.stream(self.stream):
            slab = work[:prm.passes * n * 192 * 4].view(t.float32).cpu().numpy().reshape(prm.passes, n, 192)
            out = buf.cpu().numpy().reshape(n, 192)
        self.stream.synchronize()
        return out, slab

    def scatter(self, d_buf, tiles, win, out):
        """pt_untile_list of a device tile buffer into the device tensor `out` (the window's buffer)."""
        ptamd.untile_list(d_buf.data_ptr(), tiles, self.cam, win, out.data_ptr(), self.stream.cuda_stream)

    def pattern(self, h, w):
        t = self.torch
        with t.cuda.stream(self.stream):
            return t.full((h, w, 3), PATTERN, dtype=t.int32, device=self.dev).view(t.float32)

    def host(self, x):
        with self.torch.cuda.stream(self.stream):
            h = x.cpu().numpy()
        self.stream.synchronize()
        return h


@pytest.mark.gpu
@pytest.mark.parametrize("tail", ["tail_in_wf_drain", "pipeline_to_the_end"])
@pytest.mark.parametrize("name", list(SCENES))
def test_window_is_the_crop_of_the_frame(_gpu, monkeypatch, name, tail):
    """With the library's default hand-over of the last live streams to wf_drain, and with the pipeline running to the last stream
    (PTAMD_DRAIN=0, read when a scene is created)."""
    if tail == "pipeline_to_the_end":
        monkeypatch.setenv("PTAMD_DRAIN", "0")
    else:
        monkeypatch.delenv("PTAMD_DRAIN", raising=False)
    sc = _scene(name)
    for W, H in FRAMES:
        cam, prm = ptamd.make_camera(W, H), params()
        frame = sc.render(cam, prm)
        for win in windows(W, H):
            x0, y0, x1, y1 = win
            got = sc.render_window(cam, prm, win)
            assert got.shape == (y1 - y0, x1 - x0, 3)
            assert np.array_equal(bits(got), bits(frame[y0:y1, x0:x1])), (name, W, H, win)
        # prm.rank / world are ignored as pt_render ignores them
        assert np.array_equal(bits(sc.render_window(cam, params(rank=1, world=2), (5, 3, 37, 29))), bits(frame[3:29, 5:37]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_window_matches_the_oracles_window_render(_gpu, name):
    import oracle_lib as O
    nodes, tris, _ = ptamd.build_bvh(_prims(name))
    so, sg = O.Scene(nodes.tobytes(), tris), ptamd.Scene(nodes, tris)
    for W, H in FRAMES:
        cam, prm = ptamd.make_camera(W, H), params()
        for win in windows(W, H):
            _check_against_oracle(sg.render_window(cam, prm, win), so, W, H, win, prm, f"{name} {W}x{H} window {win}", 8)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_list_order_does_not_matter_and_means_are_the_frames(_gpu, name):
    """Tile k's 192 floats are the same wherever it stands in a list and equal tile k of pt_render_tiles(world = 1); the per-pass
    means at the start of the work buffer equal, tile by tile and pass by pass, those the full-frame call leaves."""
    sc = _scene(name)
    rs = np.random.RandomState(11)
    for W, H in FRAMES:
        cam, prm = ptamd.make_camera(W, H), params()
        dv = Device(sc, cam)
        full, full_slab = dv.full(prm)
        n_total = dv.n_total
        subset = np.sort(rs.choice(n_total, n_total // 3, replace=False)).astype(np.int32)
        subset[-1] = n_total - 1                                            # always the last tile (ragged on both edges in 100 x 52)
        subset = np.unique(subset)
        for order in (subset, subset[::-1], rs.permutation(subset), np.arange(n_total, dtype=np.int32), subset[:1]):
            got, slab = dv.listed(prm, order)
            assert np.array_equal(bits(got), bits(full[order])), (name, W, H, order[:6])
            assert np.array_equal(bits(slab), bits(full_slab[:, order])), (name, W, H, order[:6])
            # d_tiles is the sum of the means in pass order starting from 0
            acc = np.zeros_like(got)
            for p in range(prm.passes):
                acc = acc + slab[p]
            assert np.array_equal(bits(acc), bits(got))
        # pixels outside the frame are exactly 0 (positive zero)
        last = dv.listed(prm, [n_total - 1])[0].reshape(8, 8, 3)
        vh, vw = H - (H - 1) // 8 * 8, W - (W - 1) // 8 * 8
        assert not bits(last[vh:]).any() and not bits(last[:, vw:]).any()
        # the numpy wrapper
        t3 = sc.render_tile_list(cam, prm, subset[::-1])
        assert t3.shape == (subset.size, 8, 8, 3) and np.array_equal(bits(t3.reshape(-1, 192)), bits(full[subset[::-1]]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_untile_list_writes_the_listed_tiles_only(_gpu, name):
    sc = _scene(name)
    rs = np.random.RandomState(5)
    for W, H in FRAMES:
        cam, prm = ptamd.make_camera(W, H), params()
        frame = sc.render(cam, prm)
        dv = Device(sc, cam)
        n_total, tiles_x = dv.n_total, (W + 7) // 8
        perm = rs.permutation(n_total).astype(np.int32)
        a, b = perm[:n_total // 2], perm[n_total // 2:]
        buf_a, buf_b = dv.listed(prm, a, keep=True), dv.listed(prm, b, keep=True)
        py, px = np.mgrid[0:H, 0:W]
        tile_of = (py // 8) * tiles_x + px // 8
        in_a = np.isin(tile_of, a)
        for win in ((0, 0, W, H), (5, 3, 37, 29), (W - 13, H - 9, W, H)):
            x0, y0, x1, y1 = win
            out = dv.pattern(y1 - y0, x1 - x0)
            dv.scatter(buf_a, a, win, out)
            got = dv.host(out)
            m = in_a[y0:y1, x0:x1]
            assert (bits(got)[~m] == PATTERN).all(), (name, W, H, win)                      # not covered by the list: not written
            assert np.array_equal(bits(got)[m], bits(frame[y0:y1, x0:x1])[m]), (name, W, H, win)
            if win == (0, 0, W, H):
                dv.scatter(buf_b, b, win, out)                                              # the complement completes the frame
                assert np.array_equal(bits(dv.host(out)), bits(frame)), (name, W, H)


@pytest.mark.gpu
def test_list_render_has_no_side_effects_and_ignores_the_mode(_gpu):
    sc = _scene("standin")
    W, H = 100, 52
    cam, prm = ptamd.make_camera(W, H), params()
    win = (5, 3, 37, 29)
    before = sc.render(cam, prm)
    want = sc.render_window(cam, prm, win)
    assert np.array_equal(bits(want), bits(before[3:29, 5:37]))
    assert np.array_equal(bits(sc.render(cam, prm)), bits(before))
    sc.set_mode(0)
    assert np.array_equal(bits(sc.render_window(cam, prm, win)), bits(want))
    sc.render_timings(reset=True)
    assert np.array_equal(bits(sc.render(cam, prm)), bits(before))
    assert sc.render_timings(reset=False).size == 1                                         # ... and that render was one render_units launch
    sc.enable_counters(True)
    assert np.array_equal(bits(sc.render_window(cam, prm, win)), bits(want))
    assert np.array_equal(bits(sc.render(cam, prm)), bits(before)) and sc.counters()[5] > 0     # the counting build still follows its switch
    sc.enable_counters(False)
    sc.set_mode(1)
    # a longer list after a shorter one (the scene's list buffer grows) and a shorter one again
    dv = Device(sc, ptamd.make_camera(1024, 1024))
    p1 = ptamd.default_params(passes=1, spp_per_pass=1)
    big = np.arange(dv.n_total, dtype=np.int32)[::5]
    assert big.size > 1024
    full, _ = dv.full(p1)
    for order in (big[:7], big, big[:3]):
        assert np.array_equal(bits(dv.listed(p1, order)[0]), bits(full[order]))
    assert np.array_equal(bits(sc.render(cam, prm)), bits(before))


def _window_by_device_calls(sc, cam, prm, win):
    dv = Device(sc, cam)
    tiles = ptamd.tiles_of_window(cam, win)
    buf = dv.listed(prm, tiles, keep=True)                  # work buffer: exactly pt_tile_list_work_bytes
    out = dv.pattern(win[3] - win[1], win[2] - win[0])
    dv.scatter(buf, tiles, win, out)
    return dv.host(out)


@pytest.mark.gpu
def test_window_of_the_1080p_frame(_gpu):
    """The window tests/test_gpu_parity.py::test_full_frame_1080p_window_parity_and_split cuts out of a full 1080p render."""
    import oracle_lib as O
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, 187))
    so, sg = O.Scene(nodes.tobytes(), tris), ptamd.Scene(nodes, tris)
    W, H, win = 1920, 1080, (900, 500, 964, 532)
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=1, spp_per_pass=2)
    assert ptamd.tile_list_work_bytes(cam, prm, ptamd.tiles_of_window(cam, win).size) < ptamd.work_bytes(cam, prm) // 4
    img = _window_by_device_calls(sg, cam, prm, win)
    _check_against_oracle(img, so, W, H, win, prm, "1080p window")
    assert np.array_equal(bits(sg.render_window(cam, prm, win)), bits(img))


@pytest.mark.gpu
def test_window_of_the_4k_four_instance_frame(_gpu):
    """The window tests/test_gpu_parity.py::test_config5_four_instances_deep_tree cuts out of a full 3840 x 2160 render."""
    import oracle_lib as O
    nodes, tris, depth = ptamd.build_bvh(ptamd.gen_scene(2, 187))
    assert tris.shape[0] == 278268 and depth == 21
    so, sg = O.Scene(nodes.tobytes(), tris), ptamd.Scene(nodes, tris)
    W, H, win = 3840, 2160, (1500, 1400, 1564, 1416)
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=1, spp_per_pass=2)
    assert ptamd.tiles_of_window(cam, win).size == 9 * 2
    img = _window_by_device_calls(sg, cam, prm, win)
    _check_against_oracle(img, so, W, H, win, prm, "4K window")
    assert np.array_equal(bits(sg.render_window(cam, prm, win)), bits(img))


def _read_png(path):
    b = open(path, "rb").read()
    pos, idat, ihdr = 8, b"", None
    while pos < len(b):
        n, typ = struct.unpack(">I4s", b[pos:pos + 8])
        if typ == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", b[pos + 8:pos + 8 + n])
        if typ == b"IDAT":
            idat += b[pos + 8:pos + 8 + n]
        pos += 12 + n
    W, H = ihdr[0], ihdr[1]
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + W * 3)
    assert not raw[:, 0].any()                               # the writer uses filter 0 on every row
    return raw[:, 1:].reshape(H, W, 3)


@pytest.mark.gpu
def test_cli_window(_gpu, tmp_path):
    exe = os.path.join(ROOT, "pathtrace-on-cuda_amd", "ptrender")
    W, H = 100, 52
    args = [exe, "--scene", "standin", "--lat-lon", "24", "--width", str(W), "--height", str(H), "--passes", "2", "--spp", "2"]
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d in (a, b, c):
        d.mkdir()
    plain = subprocess.run(args + ["--raw", "r.bin"], cwd=a, check=True, capture_output=True, timeout=300, text=True)
    full = _read_png(a / "result.png")
    assert full.shape == (H, W, 3)
    raw_full = np.fromfile(a / "r.bin", np.float32).reshape(H, W, 3)
    for d, extra in ((b, []), (c, ["--no-progressive"])):
        x0, y0, x1, y1 = 37, 5, 100, 31
        subprocess.run(args + extra + ["--window", f"{x0},{y0},{x1},{y1}", "--raw", "r.bin"], cwd=d, check=True, capture_output=True, timeout=300)
        png = _read_png(d / "result.png")
        assert png.shape == (y1 - y0, x1 - x0, 3) and np.array_equal(png, full[y0:y1, x0:x1])
        assert np.array_equal(bits(np.fromfile(d / "r.bin", np.float32).reshape(y1 - y0, x1 - x0, 3)), bits(raw_full[y0:y1, x0:x1]))
    # without the flag the binary behaves as before: same output lines (but for the timings), same result.png
    again = subprocess.run(args, cwd=tmp_path, check=True, capture_output=True, timeout=300, text=True)
    assert (tmp_path / "result.png").read_bytes() == (a / "result.png").read_bytes()
    strip = lambda s: [ln for ln in s.splitlines() if "time" not in ln and "kernel_ms" not in ln]      # noqa: E731
    assert strip(again.stdout) == strip(plain.stdout)
    w = ["--window", "8,8,40,24"]
    for bad in (w + ["--world", "2", "--rank", "0", "--id-file", "job.id"], w + ["--denoise", "d.png"], w + ["--aov", "a.bin"],
                w + ["--target-error", "0.1"], ["--window", "8,8,40"], ["--window", "8,8,8,24"], ["--window", "8,8,101,24"],
                ["--window", "-8,8,40,24"]):
        r = subprocess.run(args + bad, cwd=tmp_path, capture_output=True, timeout=60, text=True)
        assert r.returncode == 2, bad
