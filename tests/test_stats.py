"""Per-pixel moments over passes (pt_accumulate_passes, pt_variance), the error estimate reduced from them (pt_error_estimate) and
render-to-target (pt_render_converge): C-ABI surface and the numpy restatement on the CPU; bit-exactness, invariances, side effects,
agreement with the definition, the predictive value of the estimate and the stopping rule on the GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import stats_ref as R
import ptamd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pt_accumulate_passes", "pt_variance", "pt_error_scratch_bytes", "pt_error_estimate", "pt_render_converge")
SCENES = {"cornell": (0, 187), "standin": (1, 24)}
FRAMES = ((64, 48), (100, 52))      # whole tiles, and ragged on both edges


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: C-ABI surface (no device is touched) and the numpy restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound():
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in NEW_SYMBOLS:
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    for name in ("render_stats", "render_converge"):
        assert callable(getattr(ptamd.Scene, name))
    for name in ("accumulate_passes", "variance", "error_estimate", "error_scratch_bytes"):
        assert callable(getattr(ptamd, name))
    assert C.sizeof(ptamd.PtErrorEstimate) == 32


def test_scratch_size():
    # one 40-byte partial per block of 256 threads x 4 pixels, at most 1024 blocks
    for n, blocks in ((192, 1), (3072, 1), (3264, 2), (1920 * 1080 * 3, 1024), (64 * 48 * 3, 3)):
        assert ptamd.error_scratch_bytes(n) == 40 * blocks, n
    assert ptamd.lib().pt_error_scratch_bytes(0) == -1 and ptamd.lib().pt_error_scratch_bytes(-5) == -1
    with pytest.raises(ptamd.PtError):
        ptamd.error_scratch_bytes(0)


def test_bad_arguments_are_rejected_before_any_device_call():
    """Fake device addresses: they are never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    W, H = 16, 8
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=2)
    bc, bp = C.byref(cam), C.byref(prm)
    base = 1 << 40
    d_work, d_sum, d_m2, d_var, d_scr = (C.c_void_p(base + (i << 20)) for i in range(5))
    n = ptamd.tiles_floats(cam, prm)
    acc = [
        (None, bc, bp, 0, d_sum, d_m2),
        (d_work, None, bp, 0, d_sum, d_m2),
        (d_work, bc, None, 0, d_sum, d_m2),
        (d_work, bc, bp, -1, d_sum, d_m2),
        (d_work, bc, bp, 0, None, d_m2),
        (d_work, bc, bp, 0, d_sum, None),
        (d_work, bc, C.byref(ptamd.default_params(passes=0)), 0, d_sum, d_m2),
        (d_work, bc, C.byref(ptamd.default_params(passes=2, rank=2, world=2)), 0, d_sum, d_m2),
        (d_work, C.byref(ptamd.make_camera(1, 8)), bp, 0, d_sum, d_m2),
        (d_work, bc, bp, 2 ** 31 - 2, d_sum, d_m2),
    ]
    for i, a in enumerate(acc):
        assert l.pt_accumulate_passes(*a, None) == -1, i
    var = [(None, n, 2, d_var), (d_m2, n, 2, None), (d_m2, 0, 2, d_var), (d_m2, -4, 2, d_var), (d_m2, n, 1, d_var), (d_m2, n, 0, d_var)]
    for i, a in enumerate(var):
        assert l.pt_variance(*a, None) == -1, i
    out = ptamd.PtErrorEstimate()
    bo = C.byref(out)
    est = [
        (None, d_m2, bc, bp, 2, d_scr, bo),
        (d_sum, None, bc, bp, 2, d_scr, bo),
        (d_sum, d_m2, None, bp, 2, d_scr, bo),
        (d_sum, d_m2, bc, None, 2, d_scr, bo),
        (d_sum, d_m2, bc, bp, 1, d_scr, bo),
        (d_sum, d_m2, bc, bp, 2, None, bo),
        (d_sum, d_m2, bc, bp, 2, d_scr, None),
        (d_sum, d_m2, bc, C.byref(ptamd.default_params(rank=3, world=3)), 2, d_scr, bo),
    ]
    for i, a in enumerate(est):
        assert l.pt_error_estimate(*a, None) == -1, i
    assert "pt_error_estimate" in l.pt_last_error().decode() or "params" in l.pt_last_error().decode()
    rgb = np.zeros((H, W, 3), np.float32)
    done = C.c_int32(0)
    fake_scene = C.c_void_p(base)
    conv = [
        (None, bc, bp, 0.1, 8, ptamd._ptr(rgb), None, C.byref(done), bo),
        (fake_scene, bc, None, 0.1, 8, ptamd._ptr(rgb), None, C.byref(done), bo),
        (fake_scene, bc, bp, 0.1, 8, None, None, C.byref(done), bo),
        (fake_scene, bc, bp, 0.1, 8, ptamd._ptr(rgb), None, None, bo),
        (fake_scene, bc, bp, 0.1, 8, ptamd._ptr(rgb), None, C.byref(done), None),
        (fake_scene, bc, bp, 0.1, 1, ptamd._ptr(rgb), None, C.byref(done), bo),
        (fake_scene, bc, bp, float("nan"), 8, ptamd._ptr(rgb), None, C.byref(done), bo),
        (fake_scene, bc, bp, -1.0, 8, ptamd._ptr(rgb), None, C.byref(done), bo),
        (fake_scene, None, bp, 0.1, 8, ptamd._ptr(rgb), None, C.byref(done), bo),
        (fake_scene, bc, C.byref(ptamd.default_params(passes=0)), 0.1, 8, ptamd._ptr(rgb), None, C.byref(done), bo),
        (fake_scene, C.byref(ptamd.make_camera(4096, 4096)), bp, 0.1, 1000, ptamd._ptr(rgb), None, C.byref(done), bo),      # seed limit
    ]
    for i, a in enumerate(conv):
        assert l.pt_render_converge(*a) == -1, i


def _stacks(n, rs, width=256):
    rnd = (rs.uniform(0, 1, (n, width)) ** 4).astype(np.float32)
    near = (15.01 + 1e-4 * rs.standard_normal((n, width))).astype(np.float32)
    const = np.ascontiguousarray(np.broadcast_to(rs.uniform(0, 20, width).astype(np.float32), (n, width)))
    return rnd, near, const


def _m2_f64(x):
    return x.astype(np.float64).var(0) * x.shape[0]


def test_fold_against_float64_variance():
    """The float32 fold against numpy's float64 var(ddof=0) * n, n = 2 .. 257: 1e-5 relative (per float) on random stacks,
    |M2 - ref| <= 1e-9 n mean^2 on nearly constant (15.01 + 1e-4 gaussian) and on constant ones."""
    rs = np.random.RandomState(7)
    worst = [0.0, 0.0, 0.0]
    for n in range(2, 258):
        rnd, near, const = _stacks(n, rs)
        S, M2 = R.fold(rnd)
        ref = _m2_f64(rnd)
        worst[0] = max(worst[0], float((np.abs(M2 - ref) / ref).max()))
        assert np.array_equal(bits(S), bits(np.add.accumulate(rnd, 0, dtype=np.float32)[-1]))      # S is the plain running sum
        for k, x in ((1, near), (2, const)):
            _, M2 = R.fold(x)
            scale = n * x.astype(np.float64).mean(0) ** 2
            worst[k] = max(worst[k], float((np.abs(M2 - _m2_f64(x)) / scale).max()))
    print(f"fold vs float64: random {worst[0]:.2e} relative, near-constant {worst[1]:.2e}, constant {worst[2]:.2e} of n mean^2")
    assert worst[0] <= 1e-5 and worst[1] <= 1e-9 and worst[2] <= 1e-9


def test_sum_of_squares_form_fails_the_same_bar():
    """Why Q - S^2 / n is banned: on converged pixels it misses the bar the fold meets by orders of magnitude."""
    rs = np.random.RandomState(7)
    worst = 0.0
    for n in (2, 8, 64, 257):
        _, near, const = _stacks(n, rs)
        for x in (near, const):
            scale = n * x.astype(np.float64).mean(0) ** 2
            worst = max(worst, float((np.abs(R.sumsq_form(x) - _m2_f64(x)) / scale).max()))
    assert worst > 1e-7, worst      # 100 times over the bar of 1e-9


def test_fold_is_split_invariant_and_restatement_handles_nan():
    rs = np.random.RandomState(3)
    x = (rs.uniform(0, 4, (8, 50, 3)) ** 2).astype(np.float32)
    S, M2 = R.fold(x)
    for split in ((4, 4), (1, 7), (3, 3, 2), (1,) * 8):
        s = m = None
        k = 0
        for b in split:
            s, m = R.fold(x[k:k + b], s, m, k)
            k += b
        assert np.array_equal(bits(s), bits(S)) and np.array_equal(bits(m), bits(M2)), split
    x[2, 7, 1] = np.nan
    S2, M22 = R.fold(x)
    e = R.estimate(S2, M22, 8)
    keep = np.delete(np.arange(50), 7)
    assert e["skipped"] == 1 and e["pixels"] == 49 and e == {**R.estimate(S[keep], M2[keep], 8), "skipped": 1}
    v = R.variance(np.float32([-1e-9, 2.0, np.nan]), 5)
    assert v[0] == 0 and v[1] == np.float32(2.0) * np.float32(5) / np.float32(4) and np.isnan(v[2])


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    yield


class Moments:
    """Device buffers of one (scene, camera, rank, world) and the render + fold loop over batches of passes."""

    def __init__(self, sc, cam, spp, rank=0, world=1, max_batch=8, **kw):
        import torch
        self.torch, self.sc, self.cam, self.spp, self.kw = torch, sc, cam, spp, dict(rank=rank, world=world, **kw)
        self.world = world
        dev = torch.device("cuda:0")
        big = self.params(max_batch, 0)
        self.n = ptamd.tiles_floats(cam, big)
        self.tiles, self.S, self.M2, self.var = (torch.empty(self.n, dtype=torch.float32, device=dev) for _ in range(4))
        self.work = torch.empty(max(ptamd.work_bytes(cam, self.params(b, 0)) for b in range(1, max_batch + 1)), dtype=torch.uint8, device=dev)
        self.scratch = torch.empty(ptamd.error_scratch_bytes(self.n), dtype=torch.uint8, device=dev)
        self.stream = torch.cuda.Stream(dev)
        self.done = 0

    def params(self, passes, first_pass):
        return ptamd.default_params(passes=passes, spp_per_pass=self.spp, first_pass=first_pass, **self.kw)

    def add(self, passes, first_pass=0, poke=None):
        """Render `passes` more passes and fold them; poke(slab) may edit the per-pass means (passes, n) before the fold."""
        st = self.stream.cuda_stream
        prm = self.params(passes, first_pass + self.done)
        self.sc.render_tiles(self.cam, prm, self.tiles.data_ptr(), self.work.data_ptr(), st)
        if poke is not None:
            with self.torch.cuda.stream(self.stream):
                poke(self.work[:passes * self.n * 4].view(self.torch.float32).view(passes, self.n))
        ptamd.accumulate_passes(self.work.data_ptr(), self.cam, prm, self.done, self.S.data_ptr(), self.M2.data_ptr(), st)
        self.done += passes
        return self

    def run(self, split, first_pass=0, poke=None):
        self.done = 0
        for b in split:
            self.add(b, first_pass, poke)
        return self

    def variance_tiles(self):
        ptamd.variance(self.M2.data_ptr(), self.n, self.done, self.var.data_ptr(), self.stream.cuda_stream)
        with self.torch.cuda.stream(self.stream):
            out = self.var.clone()
        self.stream.synchronize()
        return out

    def estimate(self):
        return ptamd.error_estimate(self.S.data_ptr(), self.M2.data_ptr(), self.cam, self.params(1, 0), self.done,
                                    self.scratch.data_ptr(), self.stream.cuda_stream)

    def frame(self, t):
        """Tile buffer of a whole-frame (world 1) run -> (H, W, 3) numpy."""
        assert self.world == 1
        return untile_frames(self.torch, [t], self.cam, 1, self.stream)

    def host(self):
        """(S, M2) as (H, W, 3) float32."""
        return self.frame(self.S), self.frame(self.M2)


def untile_frames(torch, parts, cam, world, stream):
    """Rank-major tile buffers -> (H, W, 3) numpy; every device operation on `stream`, after the work queued there."""
    with torch.cuda.stream(stream):
        g = torch.cat(parts)
        out = torch.empty((cam.H, cam.W, 3), dtype=torch.float32, device=g.device)
        ptamd.untile(g.data_ptr(), cam, world, out.data_ptr(), stream.cuda_stream)
        host = out.cpu().numpy()
    stream.synchronize()
    return host


def _scene(name):
    kind, lat_lon = SCENES[name]
    return ptamd.Scene.from_prims(ptamd.gen_scene(kind, lat_lon))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_fold_is_bit_exact(_gpu, name):
    """Frames of one pass per call are the pass means (0 + m); folded on the host in float32 they equal S and M2 of one 8-pass call."""
    sc = _scene(name)
    for W, H in FRAMES:
        cam = ptamd.make_camera(W, H)
        means = np.stack([sc.render(cam, ptamd.default_params(passes=1, spp_per_pass=4, first_pass=j)) for j in range(8)])
        S, M2 = R.fold(means)
        gs, gm = Moments(sc, cam, 4).run((8,)).host()
        assert np.array_equal(bits(gs), bits(S)), (name, W, H)
        assert np.array_equal(bits(gm), bits(M2)), (name, W, H, np.argwhere(bits(gm) != bits(M2))[:5])
        assert (M2 > 0).mean() > 0.5
        rgb, var = sc.render_stats(cam, ptamd.default_params(passes=8, spp_per_pass=4))
        assert np.array_equal(bits(rgb), bits(S)) and np.array_equal(bits(var), bits(R.variance(M2, 8))), (name, W, H)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_fold_is_invariant_to_the_split_and_the_render_mode(_gpu, name):
    sc = _scene(name)
    for W, H in FRAMES:
        cam = ptamd.make_camera(W, H)
        frame = sc.render(cam, ptamd.default_params(passes=8, spp_per_pass=4))
        mo = Moments(sc, cam, 4)
        want = None
        for mode in (1, 0):
            sc.set_mode(mode)
            for split in ((8,), (4, 4), (1, 7), (3, 3, 2)):
                S, M2 = mo.run(split).host()
                if want is None:
                    want = (S, M2)
                    assert np.array_equal(bits(S), bits(frame)), (name, W, H)
                assert np.array_equal(bits(S), bits(want[0])) and np.array_equal(bits(M2), bits(want[1])), (name, W, H, mode, split)
        sc.set_mode(1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_variance_is_invariant_to_the_tile_split(_gpu, name):
    import torch
    sc = _scene(name)
    for W, H in FRAMES:
        cam = ptamd.make_camera(W, H)
        base = Moments(sc, cam, 4).run((5,))
        want = base.frame(base.variance_tiles())
        e1 = base.estimate()
        assert e1["pixels"] + e1["skipped"] == W * H
        for world in (2, 3):
            ranks = [Moments(sc, cam, 4, rank=r, world=world).run((2, 3)) for r in range(world)]
            got = untile_frames(torch, [m.variance_tiles() for m in ranks], cam, world, ranks[0].stream)
            assert np.array_equal(bits(got), bits(want)), (name, W, H, world)
            es = [m.estimate() for m in ranks]
            assert sum(e["pixels"] for e in es) == e1["pixels"] and sum(e["skipped"] for e in es) == e1["skipped"], (name, W, H, world)


@pytest.mark.gpu
def test_stats_calls_have_no_side_effects(_gpu):
    sc = _scene("standin")
    W, H = 100, 52
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=3, spp_per_pass=4)
    before = sc.render(cam, prm)
    mo = Moments(sc, cam, 4)
    mo.add(3)
    mo.stream.synchronize()
    state = (sc.last_iterations(), sc.counters().tolist(), sc.render_timings(reset=False).tolist(), sc.last_render_ms())
    tiles0, work0 = mo.tiles.clone(), mo.work.clone()
    ptamd.accumulate_passes(mo.work.data_ptr(), cam, mo.params(3, 0), 3, mo.S.data_ptr(), mo.M2.data_ptr(), mo.stream.cuda_stream)
    mo.done = 6
    mo.variance_tiles()
    e1, e2 = mo.estimate(), mo.estimate()
    assert e1 == e2
    assert (sc.last_iterations(), sc.counters().tolist(), sc.render_timings(reset=False).tolist(), sc.last_render_ms()) == state
    import torch
    assert torch.equal(mo.tiles.view(torch.int32), tiles0.view(torch.int32)) and torch.equal(mo.work, work0)      # inputs are only read
    assert np.array_equal(bits(sc.render(cam, prm)), bits(before))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_estimate_matches_its_definition(_gpu, name):
    from ptamd.dist import untile_index
    sc = _scene(name)
    for W, H in FRAMES:
        cam = ptamd.make_camera(W, H)
        mo = Moments(sc, cam, 4).run((8,))
        S, M2 = mo.host()
        got, again, want = mo.estimate(), mo.estimate(), R.estimate(S, M2, 8)
        exact = R.estimate32(mo.S.cpu().numpy(), mo.M2.cpu().numpy(), 8, W, H)
        print(f"{name} {W}x{H}: {got} | restatement {want}")
        assert got == again                                                       # same bits, run after run
        assert got == exact, (name, W, H, got, exact)                             # the kernel's own order, restated: same bits
        assert got["pixels"] + got["skipped"] == W * H and (got["pixels"], got["skipped"]) == (want["pixels"], want["skipped"])
        bound = R.summation_bound(mo.n, want["pixels"])                           # against the float64 definition: what the two orders explain
        for k in ("rel_rms", "mean_rel_se"):
            assert abs(got[k] - want[k]) <= bound * want[k], (name, W, H, k, got[k], want[k], bound)
        # a NaN in one pass mean of one pixel: that pixel is skipped, the figures are those of the frame without it
        fin = np.argwhere(np.isfinite(S).all(-1) & np.isfinite(M2).all(-1) & (S.sum(-1) > 0))
        py, px = fin[len(fin) // 2]
        at = int(untile_index(W, H, 1)[py * W + px]) * 3 + 1

        def poke(slab):
            slab[5, at] = float("nan")

        mo.run((8,), poke=poke)
        S2, M22 = mo.host()
        assert np.isnan(S2[py, px, 1]) and np.isnan(M22[py, px, 1])
        keep = np.ones((H, W), bool)
        keep[py, px] = False
        assert np.array_equal(bits(S2[keep]), bits(S[keep])) and np.array_equal(bits(M22[keep]), bits(M2[keep]))
        got2, want2 = mo.estimate(), R.estimate(S[keep], M2[keep], 8)
        assert got2 == R.estimate32(mo.S.cpu().numpy(), mo.M2.cpu().numpy(), 8, W, H), (name, W, H, got2)
        assert (got2["pixels"], got2["skipped"]) == (want2["pixels"], want["skipped"] + 1) and got2["pixels"] == got["pixels"] - 1
        for k in ("rel_rms", "mean_rel_se"):
            assert abs(got2[k] - want2[k]) <= bound * want2[k], (name, W, H, k, got2[k], want2[k], bound)


def _estimates_at(sc, cam, spp, batches, first_pass=0):
    """Fold `batches` (a tuple of batch sizes) and return the moments object and the estimate after each batch."""
    mo = Moments(sc, cam, spp, max_batch=max(batches))
    mo.done = 0
    out = []
    for b in batches:
        mo.add(b, first_pass)
        out.append(mo.estimate() if mo.done >= 2 else None)
    return mo, out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_estimate_predicts_the_error(_gpu, name):
    """With p the frame's rel_rms estimate, p_ref the reference's and m the measured relative RMS between them:
    0.8 <= m / sqrt(p^2 + p_ref^2) <= 1.25.  Measured on the MI355X (the CPU oracle gives the same frames bit for bit):
    Cornell 1.020 / 0.965 / 0.927, stand-in (lat_lon 24) 0.990 / 0.947 / 0.921 for 4 x 1, 8 x 4, 8 x 32 spp."""
    sc = _scene(name)
    cam = ptamd.make_camera(128, 128)
    ref_mo, (ref_est,) = _estimates_at(sc, cam, 256, (16,), first_pass=8)
    ref = ref_mo.host()[0]
    for passes, spp in ((4, 1), (8, 4), (8, 32)):
        mo, (est,) = _estimates_at(sc, cam, spp, (passes,))
        frame = mo.host()[0]
        p, p_ref = est["rel_rms"], ref_est["rel_rms"]
        m = D.rel_rms_finite(frame / passes, ref / 16)
        ratio = m / np.hypot(p, p_ref)
        print(f"{name} {passes} x {spp} spp: p {p:.4f}, p_ref {p_ref:.4f}, measured {m:.4f}, ratio {ratio:.3f}, mean_rel_se {est['mean_rel_se']:.4f}")
        assert 0.8 <= ratio <= 1.25, (name, passes, spp, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_render_converge_stops_at_the_target(_gpu, name):
    sc = _scene(name)
    cam = ptamd.make_camera(128, 128)
    mo, ests = _estimates_at(sc, cam, 4, (4,) * 16)
    p8, p16 = ests[1]["rel_rms"], ests[3]["rel_rms"]
    assert p16 < p8
    target = float(np.sqrt(p8 * p16))
    prm = ptamd.default_params(passes=4, spp_per_pass=4)
    rgb, var, done, est = sc.render_converge(cam, prm, target, 64)
    print(f"{name}: 8-pass estimate {p8:.4f}, 16-pass {p16:.4f}, target {target:.4f} -> {done} passes, estimate {est}")
    assert done % 4 == 0 and 4 <= done <= 64
    assert est["rel_rms"] <= target and est == ests[done // 4 - 1]
    if done > 4:
        assert ests[done // 4 - 2]["rel_rms"] > target
    assert all(e["rel_rms"] > target for e in ests[:done // 4 - 1])
    assert np.array_equal(bits(rgb), bits(sc.render(cam, ptamd.default_params(passes=done, spp_per_pass=4))))
    again = Moments(sc, cam, 4, max_batch=done).run((done,))
    assert np.array_equal(bits(var), bits(again.frame(again.variance_tiles())))
    # a target that cannot be reached: stops at max_passes exactly, also when it is not a multiple of the batch
    for batch, cap in ((4, 12), (4, 10), (1, 3), (8, 5)):
        rgb, var, done, est = sc.render_converge(cam, ptamd.default_params(passes=batch, spp_per_pass=2), 1e-9, cap)
        assert done == cap and est["rel_rms"] > 1e-9, (batch, cap)
        assert np.array_equal(bits(rgb), bits(sc.render(cam, ptamd.default_params(passes=cap, spp_per_pass=2)))), (batch, cap)
    # first_pass is honoured
    rgb, _, done, _ = sc.render_converge(cam, ptamd.default_params(passes=2, spp_per_pass=2, first_pass=5), 1e-9, 4)
    assert done == 4 and np.array_equal(bits(rgb), bits(sc.render(cam, ptamd.default_params(passes=4, spp_per_pass=2, first_pass=5))))


@pytest.mark.gpu
def test_cli_target_error(_gpu, tmp_path):
    exe = os.path.join(ROOT, "pathtrace-on-cuda_amd", "ptrender")
    W, H = 96, 64
    args = [exe, "--scene", "cornell", "--width", str(W), "--height", str(H), "--passes", "2", "--spp", "2", "--no-progressive"]
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d in (a, b, c):
        d.mkdir()
    plain = subprocess.run(args, cwd=a, check=True, capture_output=True, timeout=300, text=True)
    sc = _scene("cornell")
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=2, spp_per_pass=2)
    assert "Converge" not in plain.stdout
    # an unreachable target: all of --max-passes
    r = subprocess.run(args + ["--target-error", "1e-9", "--max-passes", "5", "--variance", "v.bin", "--raw", "r.bin"], cwd=b, check=True,
                       capture_output=True, timeout=300, text=True)
    rgb, var, done, est = sc.render_converge(cam, prm, 1e-9, 5)
    assert done == 5 and "Converge : passes 5 of at most 5" in r.stdout and "mean_rel_se" in r.stdout
    assert (b / "v.bin").read_bytes() == var.tobytes() and (b / "r.bin").read_bytes() == rgb.tobytes()
    assert (b / "result.png").stat().st_size > 0
    # a loose target: one batch, and with the same passes the frame — and result.png — of the plain run
    r = subprocess.run(args + ["--target-error", "1e9", "--variance", "v.bin", "--denoise", "d.png"], cwd=c, check=True, capture_output=True,
                       timeout=300, text=True)
    assert "Converge : passes 2 of at most 16" in r.stdout
    assert (c / "result.png").read_bytes() == (a / "result.png").read_bytes() and (c / "d.png").stat().st_size > 0
    assert (c / "v.bin").read_bytes() == sc.render_stats(cam, prm)[1].tobytes()
    # without the new options the binary behaves as before: same output lines (but for the timings), same result.png
    again = subprocess.run(args, cwd=tmp_path, check=True, capture_output=True, timeout=300, text=True)
    assert (tmp_path / "result.png").read_bytes() == (a / "result.png").read_bytes()
    strip = lambda s: [ln for ln in s.splitlines() if "time" not in ln and "kernel_ms" not in ln]      # noqa: E731
    assert strip(again.stdout) == strip(plain.stdout)
    bad = subprocess.run(args + ["--variance", "v.bin"], cwd=tmp_path, capture_output=True, timeout=60, text=True)
    assert bad.returncode == 2
