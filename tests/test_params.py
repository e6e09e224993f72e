"""Parity at the corners of the render parameters: rr_floor, rr_bounce, max_refract, max_bounce, spp_per_pass (rows: params_ref.ROWS).

CPU part, oracle alone: every row's frame depends on its parameter (it differs from its neighbour row's frame in at least the row's
share of pixels), the identities the reference's own arithmetic implies hold bit for bit, and the two pane stacks that would NOT
tell max_refract 249 from 250 are shown not to.  These are premises about the inputs and would need no change if the library were
rewritten.

GPU part: every row on every integrator and schedule, the sample limit, the other pixel sources, and the limits at every render entry
point.  Bits everywhere, NaN equal to NaN, no tolerances: the frames have at most 3,840 pixels."""
import ctypes as C
import time

import numpy as np
import pytest

import params_ref as P
import ptamd

_FRAMES = {}
REFUSED = (("max_refract", 251), ("max_refract", -1), ("max_bounce", 256), ("max_bounce", 0), ("spp_per_pass", 65536), ("spp_per_pass", 0))


def oracle(row_id):
    """The oracle's frame of a row, computed once per process."""
    if row_id not in _FRAMES:
        t0 = time.time()
        _FRAMES[row_id] = P.oracle_frame(P.BY_ID[row_id])
        print(f"oracle {row_id}: {time.time() - t0:.2f} s")
    return _FRAMES[row_id]


def view(row_id):
    """A row's frame cut to the window the oracle rendered."""
    row = P.BY_ID[row_id]
    return oracle(row_id) if row.window is None else P.crop(oracle(row_id), row.window)


def _assert_same(got, want, what):
    same = P.same_pixels(got, want)
    print(f"{what}: pixels with the oracle's bits {same.mean():.6f} of {same.size}")
    assert np.shape(got) == np.shape(want) and same.all(), what


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the premises
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [r for r in P.ROWS if r.finite], ids=lambda r: r.id)
def test_oracle_frame_is_finite_and_differs_from_its_neighbours(row):
    img = view(row.id)
    assert np.isfinite(img).all(), row.id
    assert img.max() > 0.0
    if row.neighbour is not None:
        share = P.share_that_differs(img, view(row.neighbour))
        print(f"{row.id} against {row.neighbour}: share of pixels that differ {share:.3f} (at least {row.min_share})")
        assert share >= row.min_share, (row.id, row.neighbour, share)


def test_oracle_identities():
    """What the reference's arithmetic implies, bit for bit: a negative floor is a floor of 0 (the select-style max returns the other
    operand, which is never negative), a roulette that starts before bounce 0 starts at bounce 0, and one that starts at max_bounce
    never runs.  And the one pair that must NOT be equal: a NaN floor ends every path at the roulette, a floor of 0 only those the
    weight says (fmaxf in place of the select would make them equal)."""
    for a, b in (("rr_floor_neg1", "rr_floor_0"), ("rr_bounce_neg5", "rr_bounce_0"), ("rr_bounce_8", "rr_bounce_1000")):
        assert P.same_pixels(oracle(a), oracle(b)).all(), (a, b)
    share = P.share_that_differs(oracle("rr_floor_nan"), oracle("rr_floor_0"))
    print(f"rr_floor NaN against 0: share of pixels that differ {share:.3f} (at least 0.04; 0.158 when the rows were chosen)")
    assert share >= 0.04


def test_a_pane_stack_needs_its_small_specular():
    """Lost discrimination, documented: with make_prims' specular 0.04 Fresnel reflection takes the paths off the straight line long
    before sheet 250 and max_refract 249 and 250 give the same frame; with specular 0 every pixel of the oracle's frame that looks
    through the stack is NaN.  Hence 0.0004."""
    a, b = oracle("spec04_refract_249"), oracle("spec04_refract_250")
    assert np.isfinite(a).all() and np.isfinite(b).all()
    share = P.share_that_differs(a, b)
    print(f"specular 0.04, max_refract 249 against 250: share of pixels that differ {share:.3f}")
    assert share == 0.0
    nan = np.isnan(oracle("spec0_refract_250")).all(-1)
    print(f"specular 0: NaN in {nan.mean():.3f} of the pixels")
    assert nan[5:18, 8:22].all()      # the block of pixels whose every sample looks through the stack


def test_both_parameter_sets_are_the_same():
    """params_pair gives the oracle and the library the same numbers, and the defaults it fills in are pt_params_default's."""
    d = ptamd.default_params()
    base = P.row_fields(P.Row("x", "standin", {}, None, 0.0))
    for k in ("max_bounce", "rr_bounce", "rr_floor", "max_refract", "first_pass"):
        assert getattr(d, k) == base[k], k
    for row in P.ROWS:
        op, gp = P.params_pair(row)
        for k in ("passes", "spp_per_pass", "max_bounce", "rr_bounce", "max_refract", "first_pass"):
            assert getattr(op, k) == getattr(gp, k) == P.row_fields(row)[k], (row.id, k)
        assert np.float32(op.rr_floor).tobytes() == np.float32(gp.rr_floor).tobytes(), row.id
        assert (gp.rank, gp.world) == (0, 1)


def test_accepted_edges_and_refusals_without_a_device():
    """The range check every render entry point starts with (pt_work_bytes runs it and touches no device): the edges 0 and 250, 1 and
    255, 1 and 65535 are accepted, one step past each is refused with a message that names the field."""
    l = ptamd.lib()
    cam = ptamd.make_camera(8, 8)
    for field, values in (("max_refract", (0, 250)), ("max_bounce", (1, 255)), ("spp_per_pass", (1, 65535))):
        for v in values:
            assert ptamd.work_bytes(cam, ptamd.default_params(**{field: v})) > 0, (field, v)
    for field, v in REFUSED:
        assert l.pt_work_bytes(C.byref(cam), C.byref(ptamd.default_params(**{field: v}))) == -1, (field, v)
        assert f"{field}={v}" in l.pt_last_error().decode(), (field, v)
    for v in (P.NAN, P.INF, -1.0, 2.0):      # not validated, and not to be
        assert ptamd.work_bytes(cam, ptamd.default_params(rr_floor=v)) > 0, v


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu
BIG = 1 << 30      # a drain threshold above every stream count: wf_drain takes every stream at the first poll
# name -> mode, shade rounds, early shade (True: the render's own stream count), drain threshold
SCHEDULES = {
    "one_kernel": (0, -1, False, 0),
    "two_rounds_pipeline_to_the_end": (1, 1, False, 0),
    "two_rounds_wf_drain": (1, 1, False, BIG),
    "one_round_pipeline_to_the_end": (1, 0, False, 0),
    "one_round_wf_drain": (1, 0, False, BIG),
    "early_shade": (1, 1, True, 0),
}
ITERATION_ROWS = ("mirror_bounce_255", "panes256_refract_250")


@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    yield


_SCENES = {}


def scheduled_scene(name):
    """One uploaded scene per scene name for the schedule tests: every test sets all four knobs."""
    if name not in _SCENES:
        nodes, tris, sph = P.built(name)
        _SCENES[name] = ptamd.Scene(nodes, tris, sph)
    return _SCENES[name]


def fresh_scene(name):
    """A scene in the default schedule."""
    nodes, tris, sph = P.built(name)
    return ptamd.Scene(nodes, tris, sph)


def n_streams(row):
    f, fields = P.FRAMES[row.scene], P.row_fields(row)
    return ((f.W + 7) // 8) * ((f.H + 7) // 8) * 64 * fields["passes"]


def iteration_bound(row):
    """hardCap (pt_wavefront.hip) without its factor 64, which is there for time-sliced traversals: these scenes have none."""
    f = P.row_fields(row)
    return f["spp_per_pass"] * (f["max_bounce"] + f["max_refract"] + 3) + 8


@gpu
@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("row", P.FRAME_ROWS, ids=lambda r: r.id)
def test_row_on_every_integrator(_gpu, row, schedule):
    """The full-frame render of a row is the oracle's frame, bit for bit, in the one-kernel mode and in every schedule of the pipeline.
    After the mirror box at max_bounce 255 and the 256 panes at max_refract 250, in the schedules without wf_drain, the pipeline has
    run at most spp * (max_bounce + max_refract + 3) + 8 iterations.


    pt_last_iterations counts launched iterations: the first poll of the live-stream count at or after the iteration that retired the
    last stream.  With wf_drain off the host polls every 16 iterations, so it is at most 15 above what the render needed (511 and 512
    in the box, 1007 and 1010 behind the panes by the counting build's per-launch ray counts).  While the host still polled every 64
    there, four of these six cases read 560 against 540 and 1072 against 1052."""
    mode, rounds, early, drain = SCHEDULES[schedule]
    sc = scheduled_scene(row.scene)
    sc.set_mode(mode)
    sc.set_shade_rounds(rounds)
    sc.set_early_shade(n_streams(row) if early else 0)
    sc.set_drain_threshold(drain)
    _, prm = P.params_pair(row)
    img = sc.render(P.cameras(row)[1], prm)      # raises unless the call returned PT_OK
    _assert_same(img, oracle(row.id), f"{row.id}, {schedule}")
    if row.id in ITERATION_ROWS and mode == 1 and drain == 0:
        it = sc.last_iterations()
        print(f"{row.id}, {schedule}: {it} iterations, bound {iteration_bound(row)}")
        assert 0 < it <= iteration_bound(row), (row.id, schedule, it)


@gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["one_kernel", "default_schedule"])
@pytest.mark.parametrize("row", P.LIMIT_ROWS, ids=lambda r: r.id)
def test_sample_limit(_gpu, row, mode):
    """spp_per_pass 32769 (bit 31 of the packed stream state is set from 32768 samples on) on one tile: 64 streams, which wf_drain takes
    at the first poll of the default schedule.  The oracle renders the window (3, 3, 5, 5).  One wave working alone: 11.5 s in the
    one-kernel mode and 5.5 s in the default schedule on an MI355X.  The limit itself, 65535, took 25.7 s and 12.1 s there (both frames
    the oracle's, bit for bit), more than the 10 s it was given, and is left to the oracle (params_ref.ROWS) and to the range check
    (test_accepted_edges_and_refusals_without_a_device)."""
    sc = fresh_scene(row.scene)
    sc.set_mode(mode)
    _, prm = P.params_pair(row)
    t0 = time.time()
    img = sc.render(P.cameras(row)[1], prm)
    print(f"{row.id}, mode {mode}: {time.time() - t0:.2f} s on the GPU")
    _assert_same(P.crop(img, row.window), view(row.id), f"{row.id}, mode {mode}")


SOURCE_ROWS = [P.BY_ID[i] for i in ("combined", "panes12_refract_10", "panes12_refract_11")]
SECOND_VIEW = dict(pos=(4.0, 22.0, 56.0), rot=(3.0, 95.0, 0.0), fovy_deg=50.0)


def tile_of(img, t):
    tx = (img.shape[1] + 7) // 8
    return img[8 * (t // tx):8 * (t // tx) + 8, 8 * (t % tx):8 * (t % tx) + 8]


@gpu
@pytest.mark.parametrize("row", SOURCE_ROWS, ids=lambda r: r.id)
def test_window_and_tile_list(_gpu, row):
    f = P.FRAMES[row.scene]
    assert f.W % 8 == 0 and f.H % 8 == 0
    sc, (_, cam), (_, prm), ref = fresh_scene(row.scene), P.cameras(row), P.params_pair(row), oracle(row.id)
    for win in ((5, 3, f.W - 3, f.H - 5), (8, 8, 24, 16), (f.W - 1, f.H - 1, f.W, f.H)):      # unaligned | whole tiles | the last pixel
        _assert_same(sc.render_window(cam, prm, win), P.crop(ref, win), f"{row.id}, window {win}")
    n_tiles = (f.W // 8) * (f.H // 8)
    tiles = [n_tiles - 1, 0, n_tiles // 2, 1]
    got = sc.render_tile_list(cam, prm, tiles)
    for i, t in enumerate(tiles):
        _assert_same(got[i], tile_of(ref, t), f"{row.id}, tile {t} of the list")


@gpu
@pytest.mark.parametrize("row", SOURCE_ROWS, ids=lambda r: r.id)
def test_two_views(_gpu, row):
    sc, (_, prm) = fresh_scene(row.scene), P.params_pair(row)
    got = sc.render_views([P.cameras(row)[1], P.cameras(row, **SECOND_VIEW)[1]], prm)
    _assert_same(got[0], oracle(row.id), f"{row.id}, view 0")
    second = P.oracle_frame(row, **SECOND_VIEW)
    assert P.share_that_differs(second, oracle(row.id)) > 0.5      # another frame altogether
    _assert_same(got[1], second, f"{row.id}, view 1")


@gpu
@pytest.mark.parametrize("row", SOURCE_ROWS, ids=lambda r: r.id)
def test_rays_of_the_camera(_gpu, row):
    """The camera's own rays and seeds (ptamd.camera_rays), pass by pass, summed in pass order as the frame is."""
    f, fields = P.FRAMES[row.scene], P.row_fields(row)
    sc, cam = fresh_scene(row.scene), P.cameras(row)[1]
    acc = np.zeros((f.W * f.H, 3), np.float32)
    for k in range(fields["passes"]):
        rays, seeds, stride = ptamd.camera_rays(cam, k)
        _, prm = P.params_pair(row, passes=1, first_pass=k)
        acc = (acc + sc.render_rays(rays, prm, seeds, stride)).astype(np.float32)
    _assert_same(acc.reshape(f.H, f.W, 3), oracle(row.id), f"{row.id}, rays")


@gpu
@pytest.mark.parametrize("row", SOURCE_ROWS, ids=lambda r: r.id)
def test_rank_1_of_3(_gpu, row):
    """A tile split: rank 1 of 3 renders the tiles t = 3 lt + 1; each is the oracle's, and the padding past the last tile is 0."""
    import torch
    from ptamd.dist import TileRenderer
    f = P.FRAMES[row.scene]
    sc, cam, ref = fresh_scene(row.scene), P.cameras(row)[1], oracle(row.id)
    _, prm = P.params_pair(row)
    prm.rank, prm.world = 1, 3
    tiles = TileRenderer(sc, cam, prm, torch.device("cuda:0")).render()
    torch.cuda.synchronize()
    got = tiles.cpu().numpy().reshape(-1, 8, 8, 3)
    n_tiles = (f.W // 8) * (f.H // 8)
    assert got.shape[0] == (n_tiles + 2) // 3
    for lt in range(got.shape[0]):
        t = 3 * lt + 1
        if t < n_tiles:
            _assert_same(got[lt], tile_of(ref, t), f"{row.id}, rank 1 of 3, tile {t}")
        else:
            assert (P.bits(got[lt]) == 0).all(), (row.id, lt)


# ---- the limits, one table for every render entry point --------------------------------------------------------------------------
ENTRY_POINTS = ("pt_render", "pt_render_tiles", "pt_render_tile_list", "pt_render_window", "pt_render_views", "pt_render_rays",
                "pt_render_adaptive", "pt_render_converge")


@gpu
def test_limits_at_every_render_entry_point(_gpu):
    """max_refract 251 and -1, max_bounce 256 and 0, spp_per_pass 65536 and 0 are refused by every render entry point, on a real scene
    with real buffers, with PT_ERR_INVALID and a message that names the field.  (The accepted edges 250 and 255 are rows above, 65535 passes the
    range check in test_accepted_edges_and_refusals_without_a_device; rr_floor is not validated, include/pt_api.h says what its odd
    values do.)"""
    import torch
    l = ptamd.lib()
    row = P.BY_ID["combined"]
    sc, cam = fresh_scene(row.scene), P.cameras(row)[1]
    ok = P.params_pair(row)[1]
    assert ok.passes == 2      # pt_render_adaptive and pt_render_converge estimate a variance across passes
    dev = torch.device("cuda:0")
    n = cam.W * cam.H
    tile_list = np.array([3, 0, 7], np.int32)
    cams = ptamd._camera_array([cam, cam])
    rays = torch.from_numpy(ptamd.camera_rays(cam, 0)[0]).to(dev)
    d_tiles = torch.zeros(max(ptamd.tiles_floats(cam, ok), ptamd.views_floats(cam, 2), ptamd.rays_floats(n)), dtype=torch.float32, device=dev)
    d_work = torch.zeros(max(ptamd.work_bytes(cam, ok), ptamd.views_work_bytes(cam, ok, 2), ptamd.rays_work_bytes(ok, n)), dtype=torch.uint8, device=dev)
    h_rgb, h_var, h_mean = (np.zeros((cam.H, cam.W, 3), np.float32) for _ in range(3))
    h_np, h_err = np.zeros(n // 64, np.int32), np.zeros(n // 64, np.float64)
    done, est, rep = C.c_int32(0), ptamd.PtErrorEstimate(), ptamd.PtAdaptiveReport()
    bc, p = C.byref(cam), ptamd._ptr
    T, Wk = C.c_void_p(d_tiles.data_ptr()), C.c_void_p(d_work.data_ptr())

    def calls(bp):
        return {
            "pt_render": lambda: l.pt_render(sc.handle, bc, bp, p(h_rgb)),
            "pt_render_tiles": lambda: l.pt_render_tiles(sc.handle, bc, bp, T, Wk, None),
            "pt_render_tile_list": lambda: l.pt_render_tile_list(sc.handle, bc, bp, p(tile_list), tile_list.size, T, Wk, None),
            "pt_render_window": lambda: l.pt_render_window(sc.handle, bc, bp, 0, 0, cam.W, cam.H, p(h_rgb)),
            "pt_render_views": lambda: l.pt_render_views(sc.handle, cams, 2, bp, None, T, Wk, None),
            "pt_render_rays": lambda: l.pt_render_rays(sc.handle, C.c_void_p(rays.data_ptr()), None, n, n, bp, T, Wk, None),
            "pt_render_adaptive": lambda: l.pt_render_adaptive(sc.handle, bc, bp, 0.5, 2, 2, p(h_rgb), p(h_mean), p(h_var), p(h_np), p(h_err), C.byref(rep)),
            "pt_render_converge": lambda: l.pt_render_converge(sc.handle, bc, bp, 0.5, 2, p(h_rgb), p(h_var), C.byref(done), C.byref(est)),
        }

    assert set(calls(C.byref(ok))) == set(ENTRY_POINTS)
    for field, value in REFUSED:
        bad = ptamd.PtParams.from_buffer_copy(ok)
        setattr(bad, field, value)
        for name, call in calls(C.byref(bad)).items():
            assert call() == -1, (name, field, value)      # PT_ERR_INVALID
            msg = l.pt_last_error().decode()
            assert f"{field}={value}" in msg, (name, field, value, msg)
    torch.cuda.synchronize()
    # the same calls with the parameters in range go through: the refusals above were the parameters', not another argument's
    for name, call in calls(C.byref(ok)).items():
        assert call() == 0, (name, l.pt_last_error().decode())
    torch.cuda.synchronize()
    _assert_same(sc.render(cam, ok), oracle(row.id), "the scene renders as before")
