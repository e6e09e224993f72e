"""Adaptive sampling (pt_accumulate_tile_list, pt_tile_errors, pt_finish_tiles, pt_render_adaptive): C-ABI surface and the numpy
restatement on the CPU; on the GPU the list fold, the per-tile error figure, the stopping loop and the CLI, all bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as A
import ptamd
from test_stats import FRAMES, Moments, _scene, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pt_accumulate_tile_list", "pt_tile_errors", "pt_finish_tiles", "pt_render_adaptive")
SPP = 4
SENTINEL = 0x7FC12345      # a NaN pattern no computation here produces


def prm_of(passes, first_pass=0, spp=SPP):
    return ptamd.default_params(passes=passes, spp_per_pass=spp, first_pass=first_pass)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: C-ABI surface (no device is touched) and the numpy restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def test_adaptive_symbols_are_exported_and_bound():
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in NEW_SYMBOLS:
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    assert callable(ptamd.Scene.render_adaptive)
    for name in ("accumulate_tile_list", "tile_errors", "finish_tiles"):
        assert callable(getattr(ptamd, name))
    assert C.sizeof(ptamd.PtTileError) == 16 and ptamd.TILE_ERROR_DTYPE.itemsize == 16
    assert C.sizeof(ptamd.PtAdaptiveReport) == 32


def test_adaptive_bad_arguments_are_rejected_before_any_device_call():
    """Fake device addresses: they are never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    W, H = 16, 8      # 2 tiles
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=2)
    bc, bp = C.byref(cam), C.byref(prm)
    base = 1 << 40
    d_work, d_sum, d_m2, d_list, d_np, d_err, d_mean, d_var = (C.c_void_p(base + (i << 20)) for i in range(8))
    small = C.byref(ptamd.make_camera(1, 8))
    acc = [
        (None, bc, bp, d_list, 2, 0, d_sum, d_m2, d_np),
        (d_work, None, bp, d_list, 2, 0, d_sum, d_m2, d_np),
        (d_work, bc, None, d_list, 2, 0, d_sum, d_m2, d_np),
        (d_work, bc, bp, None, 2, 0, d_sum, d_m2, d_np),
        (d_work, bc, bp, d_list, 2, 0, None, d_m2, d_np),
        (d_work, bc, bp, d_list, 2, 0, d_sum, None, d_np),
        (d_work, bc, bp, d_list, 0, 0, d_sum, d_m2, d_np),
        (d_work, bc, bp, d_list, -1, 0, d_sum, d_m2, d_np),
        (d_work, bc, bp, d_list, 3, 0, d_sum, d_m2, d_np),
        (d_work, bc, bp, d_list, 2, -1, d_sum, d_m2, d_np),
        (d_work, bc, bp, d_list, 2, 2 ** 31 - 2, d_sum, d_m2, d_np),
        (d_work, bc, C.byref(ptamd.default_params(passes=0)), d_list, 2, 0, d_sum, d_m2, d_np),
        (d_work, bc, C.byref(ptamd.default_params(passes=2, rank=1, world=2)), d_list, 2, 0, d_sum, d_m2, d_np),
        (d_work, bc, C.byref(ptamd.default_params(passes=2, rank=0, world=2)), d_list, 1, 0, d_sum, d_m2, d_np),
        (d_work, small, bp, d_list, 1, 0, d_sum, d_m2, d_np),
    ]
    for i, a in enumerate(acc):
        assert l.pt_accumulate_tile_list(*a, None) == -1, i
    errs = [
        (None, d_m2, bc, d_list, 2, 2, d_err),
        (d_sum, None, bc, d_list, 2, 2, d_err),
        (d_sum, d_m2, None, d_list, 2, 2, d_err),
        (d_sum, d_m2, bc, d_list, 2, 2, None),
        (d_sum, d_m2, bc, d_list, 0, 2, d_err),
        (d_sum, d_m2, bc, None, 3, 2, d_err),
        (d_sum, d_m2, bc, d_list, 2, 1, d_err),
        (d_sum, d_m2, bc, d_list, 2, 0, d_err),
        (d_sum, d_m2, small, d_list, 1, 2, d_err),
    ]
    for i, a in enumerate(errs):
        assert l.pt_tile_errors(*a, None) == -1, i
    fin = [
        (None, d_m2, d_np, bc, d_mean, d_var),
        (d_sum, None, d_np, bc, d_mean, d_var),
        (d_sum, d_m2, None, bc, d_mean, d_var),
        (d_sum, d_m2, d_np, None, d_mean, d_var),
        (d_sum, d_m2, d_np, bc, None, None),
        (d_sum, d_m2, d_np, small, d_mean, d_var),
    ]
    for i, a in enumerate(fin):
        assert l.pt_finish_tiles(*a, None) == -1, i
    rgb = np.zeros((H, W, 3), np.float32)
    tp = np.zeros(2, np.int32)
    rep = ptamd.PtAdaptiveReport()
    pr, pt, br = ptamd._ptr(rgb), ptamd._ptr(tp), C.byref(rep)
    fake_scene = C.c_void_p(base)
    ada = [
        (None, bc, bp, 0.1, 2, 8, pr, None, None, pt, None, br),
        (fake_scene, None, bp, 0.1, 2, 8, pr, None, None, pt, None, br),
        (fake_scene, bc, None, 0.1, 2, 8, pr, None, None, pt, None, br),
        (fake_scene, bc, bp, 0.1, 2, 8, None, None, None, pt, None, br),
        (fake_scene, bc, bp, 0.1, 2, 8, pr, None, None, None, None, br),
        (fake_scene, bc, bp, 0.1, 2, 8, pr, None, None, pt, None, None),
        (fake_scene, bc, bp, float("nan"), 2, 8, pr, None, None, pt, None, br),
        (fake_scene, bc, bp, -1.0, 2, 8, pr, None, None, pt, None, br),
        (fake_scene, bc, bp, 0.1, 9, 8, pr, None, None, pt, None, br),      # min_passes > max_passes
        (fake_scene, bc, bp, 0.1, 0, 1, pr, None, None, pt, None, br),      # min_passes is raised to 2 > max_passes
        (fake_scene, bc, C.byref(ptamd.default_params(passes=0)), 0.1, 2, 8, pr, None, None, pt, None, br),
        (fake_scene, C.byref(ptamd.make_camera(4096, 4096)), bp, 0.1, 2, 1000, pr, None, None, pt, None, br),      # seed limit
        (fake_scene, small, bp, 0.1, 2, 8, pr, None, None, pt, None, br),
    ]
    for i, a in enumerate(ada):
        assert l.pt_render_adaptive(*a) == -1, i


def test_tree_sum_against_a_plain_sum():
    """The fixed tree adds 64 non-negative float64 terms in 6 levels: within 64 * 2^-53 relative of numpy's sum (itself within that of
    the exact sum), and it is the order written down: pixel l < o adds pixel l + o."""
    rs = np.random.RandomState(11)
    x = (rs.uniform(0, 1, (500, 64)) ** 6).astype(np.float32).astype(np.float64)
    x[::7, 20:] = 0.0
    got, plain = A.tree_sum(x), x.sum(-1)
    assert (np.abs(got - plain) <= 64 * 2.0 ** -53 * plain).all()
    a = x[3].copy()
    for o in (32, 16, 8, 4, 2, 1):
        for l in range(o):
            a[l] = a[l] + a[l + o]
    assert a[0] == got[3]
    assert A.tree_sum(np.zeros(64)) == 0.0


def test_restatement_of_the_tile_error_and_the_loop():
    """A 16x8 frame of two tiles: a constant tile stops at the first check, a noisy one runs to the cap; the edge cases of the figure."""
    rs = np.random.RandomState(5)
    P, H, W = 12, 8, 16
    means = np.empty((P, H, W, 3), np.float32)
    means[:, :, :8] = np.float32(0.75)
    means[:, :, 8:] = rs.uniform(0, 2, (P, H, 8, 3)).astype(np.float32)
    for min_passes, first in ((0, 4), (2, 4), (5, 8), (9, 12)):
        r = A.adaptive_loop(means, 1e-3, 4, min_passes, 12)
        assert r["tile_passes"].tolist() == [[first, 12]], min_passes
        assert r["tile_err"][0, 0] == 0.0 and r["tile_err"][0, 1] > 1e-3
        assert r["rounds"] == 3 and r["converged"] == 1 and r["work"] == first + 12 and r["max_err"] == r["tile_err"][0, 1]
        (S_early, _), (S_all, M2_all) = A.R.fold(means[:first]), A.R.fold(means)
        assert np.array_equal(bits(r["S"][:, :8]), bits(S_early[:, :8])) and np.array_equal(bits(r["S"][:, 8:]), bits(S_all[:, 8:]))
        assert np.array_equal(bits(r["M2"][:, 8:]), bits(M2_all[:, 8:]))
    # a shortened last batch, and a cap below the batch
    assert A.adaptive_loop(means, 0.0, 4, 6, 6)["tile_passes"].tolist() == [[6, 6]]
    assert A.adaptive_loop(means, 1e30, 8, 2, 3)["tile_passes"].tolist() == [[3, 3]]
    # the figure: ragged frame, a NaN pixel, a tile of NaNs
    S, M2 = A.R.fold(rs.uniform(0, 2, (6, 12, 20, 3)).astype(np.float32))
    err, pix, skip = A.tile_errors(S, M2, 6)
    assert pix.tolist() == [64, 64, 32, 32, 32, 16] and not skip.any() and (err > 0).all()
    S2 = S.copy()
    S2[2, 9, 1] = np.nan
    S2[8:, 16:] = np.nan
    err2, pix2, skip2 = A.tile_errors(S2, M2, 6)
    assert pix2.tolist() == [64, 63, 32, 32, 32, 0] and skip2.tolist() == [0, 1, 0, 0, 0, 16] and err2[5] == 0.0
    assert err2[1] != err[1] and np.array_equal(np.delete(err2, [1, 5]), np.delete(err, [1, 5]))
    mean, var = A.finish(S, M2, np.array([[6, 3, 0], [1, 6, 6]], np.int32))
    assert np.array_equal(bits(mean[:8, :8]), bits(S[:8, :8] / np.float32(6))) and np.array_equal(bits(mean[:8, 8:16]), bits(S[:8, 8:16] / np.float32(3)))
    assert not bits(mean[:8, 16:]).any() and not bits(var[:8, 16:]).any()
    assert np.array_equal(bits(var[8:, 8:16]), bits(A.R.variance(M2[8:, 8:16], 6)))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    yield


def _tiles_of(t, cam):
    """frame-layout tile buffer (torch, n floats) -> (tiles, 192) uint32 numpy"""
    return t.cpu().numpy().view(np.uint32).reshape(-1, 192)


@pytest.mark.gpu
def test_list_fold_is_bit_exact_and_touches_only_the_list(_gpu):
    import torch
    sc = _scene("standin")
    W, H = 100, 52
    cam = ptamd.make_camera(W, H)
    ty, tx = A.tile_grid(W, H)
    total = ty * tx
    full = Moments(sc, cam, SPP).run((5,))
    full.stream.synchronize()
    wantS, wantM = _tiles_of(full.S, cam), _tiles_of(full.M2, cam)
    rs = np.random.RandomState(2)
    lst = rs.permutation(total - 1)[:total // 2 - 1].astype(np.int32)
    lst = np.insert(lst, 7, total - 1)      # the corner tile: ragged on both edges
    n = lst.size
    listed = np.zeros(total, bool)
    listed[lst] = True
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    d_list = torch.from_numpy(lst).to(dev)
    out = torch.empty(ptamd.tile_list_floats(n), dtype=torch.float32, device=dev)
    work = torch.empty(max(ptamd.tile_list_work_bytes(cam, prm_of(b), n) for b in range(1, 6)), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for split in ((5,), (2, 3), (1, 4)):
        with torch.cuda.stream(stream):
            S = torch.full((total * 192,), SENTINEL, dtype=torch.int32, device=dev)
            M2 = torch.full((total * 192,), SENTINEL, dtype=torch.int32, device=dev)
            npass = torch.full((total,), -7, dtype=torch.int32, device=dev)
        done = 0
        for b in split:
            p = prm_of(b, done)
            sc.render_tile_list_device(cam, p, lst, out.data_ptr(), work.data_ptr(), st)
            ptamd.accumulate_tile_list(work.data_ptr(), cam, p, d_list.data_ptr(), n, done, S.data_ptr(), M2.data_ptr(), npass.data_ptr(), st)
            done += b
        stream.synchronize()
        gS, gM, gn = _tiles_of(S, cam), _tiles_of(M2, cam), npass.cpu().numpy()
        assert np.array_equal(gS[listed], wantS[listed]) and np.array_equal(gM[listed], wantM[listed]), split
        assert (gS[~listed] == SENTINEL).all() and (gM[~listed] == SENTINEL).all(), split
        assert (gn[listed] == 5).all() and (gn[~listed] == -7).all(), split
    # without a pass-count buffer
    p = prm_of(5)
    sc.render_tile_list_device(cam, p, lst, out.data_ptr(), work.data_ptr(), st)
    ptamd.accumulate_tile_list(work.data_ptr(), cam, p, d_list.data_ptr(), n, 0, S.data_ptr(), M2.data_ptr(), 0, st)
    stream.synchronize()
    assert np.array_equal(_tiles_of(S, cam)[listed], wantS[listed])


def _gpu_tile_errors(mo, lst, n_passes):
    import torch
    total = mo.n // 192
    n = total if lst is None else len(lst)
    d_err = torch.zeros(n * 16, dtype=torch.uint8, device=mo.S.device)
    d_list = torch.from_numpy(np.asarray(lst, np.int32)).to(mo.S.device) if lst is not None else None
    mo.stream.wait_stream(torch.cuda.current_stream())
    ptamd.tile_errors(mo.S.data_ptr(), mo.M2.data_ptr(), mo.cam, d_list.data_ptr() if lst is not None else 0, n, n_passes, d_err.data_ptr(),
                      mo.stream.cuda_stream)
    mo.stream.synchronize()
    return d_err.cpu().numpy().view(ptamd.TILE_ERROR_DTYPE)


def _same_errors(got, want, idx=None):
    err, pix, skip = (w if idx is None else w[idx] for w in want)
    return (np.array_equal(got["mean_rel_se"].view(np.uint64), err.view(np.uint64)) and np.array_equal(got["pixels"], pix)
            and np.array_equal(got["skipped"], skip))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "standin"])
def test_tile_errors_match_the_restatement_bit_for_bit(_gpu, name):
    from ptamd.dist import untile_index
    sc = _scene(name)
    for W, H in FRAMES:
        cam = ptamd.make_camera(W, H)
        ty, tx = A.tile_grid(W, H)
        total = ty * tx
        mo = Moments(sc, cam, SPP).run((8,))
        S, M2 = mo.host()
        want = A.tile_errors(S, M2, 8)
        got = _gpu_tile_errors(mo, None, 8)
        print(f"{name} {W}x{H}: tile errors {np.sort(want[0])[[0, total // 2, -1]]}, pixels {np.unique(want[1]).tolist()}")
        assert _same_errors(got, want), (name, W, H, np.argwhere(got["mean_rel_se"] != want[0])[:5])
        assert want[1].sum() + want[2].sum() == W * H and (want[0] > 0).sum() >= total // 4
        assert got.tobytes() == _gpu_tile_errors(mo, None, 8).tobytes()                 # same bits, run after run
        lst = np.random.RandomState(4).permutation(total)[:total // 3].astype(np.int32)
        assert _same_errors(_gpu_tile_errors(mo, lst, 8), want, lst), (name, W, H)
        # a NaN in one pass mean of one pixel: that pixel is skipped; every pass mean of the last tile NaN: (0.0, 0, in-frame pixels)
        fin = np.argwhere(np.isfinite(S).all(-1) & np.isfinite(M2).all(-1) & (S.sum(-1) > 0))
        py, px = fin[len(fin) // 2]
        at = int(untile_index(W, H, 1)[py * W + px]) * 3 + 1
        t_pix = (py // 8) * tx + px // 8
        assert t_pix != total - 1

        def poke(slab):
            slab[5, at] = float("nan")
            slab[3, (total - 1) * 192:total * 192] = float("nan")

        mo.run((8,), poke=poke)
        S2, M22 = mo.host()
        want2 = A.tile_errors(S2, M22, 8)
        got2 = _gpu_tile_errors(mo, None, 8)
        assert _same_errors(got2, want2), (name, W, H)
        assert got2["skipped"][t_pix] == want[2][t_pix] + 1 and got2["pixels"][t_pix] == want[1][t_pix] - 1
        last = got2[total - 1]
        assert (last["mean_rel_se"], last["pixels"], last["skipped"]) == (0.0, 0, want[1][total - 1] + want[2][total - 1])
        others = np.ones(total, bool)
        others[[t_pix, total - 1]] = False
        assert got2[others].tobytes() == got[others].tobytes()


def _simulate(sc, cam, batch, cap):
    """The expected run from `cap` single-pass frames: the target (the midpoint between the two positive first-check tile errors that
    straddle their median) and the restatement's loop with it."""
    means = np.stack([sc.render(cam, prm_of(1, j)) for j in range(cap)])
    first = A.adaptive_loop(means, 0.0, batch, 2, batch)["checks"][0][1]
    pos = np.sort(first[first > 0])
    target = 0.5 * (pos[len(pos) // 2 - 1] + pos[len(pos) // 2])
    return means, float(target), A.adaptive_loop(means, float(target), batch, 2, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("size", FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["cornell", "standin"])
def test_adaptive_loop_matches_the_restatement(_gpu, name, size):
    sc = _scene(name)
    batch, cap = 4, 32
    for W, H in (size,):
        cam = ptamd.make_camera(W, H)
        ty, tx = A.tile_grid(W, H)
        means, target, want = _simulate(sc, cam, batch, cap)
        wp = want["tile_passes"]
        counts = dict(zip(*[v.tolist() for v in np.unique(wp, return_counts=True)]))
        print(f"{name} {W}x{H}: target {target:.6g}, tiles per pass count {counts}, mean {wp.mean():.2f} of {cap}")
        # the inputs do not let the test pass vacuously
        for done, errs in want["checks"]:
            assert (np.abs(errs - target) > 1e-9 * target).all(), (name, W, H, done)
        assert len(counts) >= (4 if (W, H) == (100, 52) else 3) and counts.get(batch, 0) >= 1 and counts.get(cap, 0) >= 1, (name, W, H, counts)

        got = sc.render_adaptive(cam, prm_of(batch), target, cap)
        assert got["tile_passes"].dtype == np.int32 and got["tile_passes"].shape == (ty, tx) and got["tile_err"].shape == (ty, tx)
        assert np.array_equal(got["tile_passes"], wp), (name, W, H, np.argwhere(got["tile_passes"] != wp)[:5])
        assert np.array_equal(got["tile_err"].view(np.uint64), want["tile_err"].view(np.uint64)), (name, W, H)
        n_pix = np.repeat(np.repeat(wp, 8, 0), 8, 1)[:H, :W]
        assert np.array_equal(bits(got["rgb"]), bits(want["S"])), (name, W, H)
        for n_t in counts:
            m = n_pix == n_t
            frame = sc.render(cam, prm_of(n_t))
            assert np.array_equal(bits(got["rgb"][m]), bits(frame[m])), (name, W, H, n_t)
            mo = Moments(sc, cam, SPP, max_batch=n_t).run((n_t,))
            var = mo.frame(mo.variance_tiles())
            assert np.array_equal(bits(got["var"][m]), bits(var[m])), (name, W, H, n_t)
            assert np.array_equal(bits(got["mean"][m]), bits(got["rgb"][m] / np.float32(n_t))), (name, W, H, n_t)
        rep = got["report"]
        assert rep["tiles"] == ty * tx and rep["tile_passes"] == int(wp.sum()) == want["work"]
        assert rep["rounds"] == want["rounds"] == int(wp.max()) // batch
        assert rep["tiles_converged"] == want["converged"] == int((got["tile_err"] <= target).sum())
        assert rep["tiles_converged"] >= int((wp < cap).sum())
        assert rep["max_tile_err"] == want["max_err"] == got["tile_err"].max()


@pytest.mark.gpu
def test_adaptive_degenerate_settings(_gpu):
    sc = _scene("standin")
    W, H = 100, 52
    cam = ptamd.make_camera(W, H)
    ty, tx = A.tile_grid(W, H)
    fixed = prm_of(3, 2)
    before = sc.render(cam, fixed)
    # no tile ever stops; the second round is shortened
    got = sc.render_adaptive(cam, prm_of(4), 1e-9, 6, min_passes=6)
    assert (got["tile_passes"] == 6).all() and got["report"]["rounds"] == 2 and got["report"]["tile_passes"] == 6 * ty * tx
    frame6 = sc.render(cam, prm_of(6))
    assert np.array_equal(bits(got["rgb"]), bits(frame6))
    assert np.array_equal(bits(got["mean"]), bits(frame6 / np.float32(6)))
    mo = Moments(sc, cam, SPP).run((6,))
    assert np.array_equal(bits(got["var"]), bits(mo.frame(mo.variance_tiles())))
    S, M2 = mo.host()
    assert np.array_equal(got["tile_err"].view(np.uint64).ravel(), A.tile_errors(S, M2, 6)[0].view(np.uint64))
    # first_pass is honoured
    got = sc.render_adaptive(cam, prm_of(4, 5), 1e-9, 6, min_passes=6)
    assert np.array_equal(bits(got["rgb"]), bits(sc.render(cam, prm_of(6, 5))))
    # a target nothing misses: every tile stops at min_passes rounded up to the batch
    for batch, min_passes, stop in ((4, 2, 4), (4, 5, 8), (2, 0, 2), (3, 7, 9)):
        got = sc.render_adaptive(cam, prm_of(batch), 1e30, 16, min_passes=min_passes)
        assert (got["tile_passes"] == stop).all() and got["report"]["tiles_converged"] == ty * tx, (batch, min_passes)
        assert got["report"]["rounds"] == stop // batch and np.array_equal(bits(got["rgb"]), bits(sc.render(cam, prm_of(stop)))), (batch, min_passes)
    # existing renders are unchanged
    assert np.array_equal(bits(sc.render(cam, fixed)), bits(before))


@pytest.mark.gpu
def test_cli_adaptive(_gpu, tmp_path):
    exe = os.path.join(ROOT, "pathtrace-on-cuda_amd", "ptrender")
    W, H = 96, 64
    args = [exe, "--scene", "cornell", "--width", str(W), "--height", str(H), "--spp", "2", "--no-progressive"]
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d in (a, b, c):
        d.mkdir()
    plain = subprocess.run(args + ["--passes", "6"], cwd=a, check=True, capture_output=True, timeout=300, text=True)
    assert "Adaptive" not in plain.stdout
    # no tile ever stops: the frame, and result.png, of the plain run
    r = subprocess.run(args + ["--passes", "2", "--adaptive", "1e-9", "--min-passes", "6", "--max-passes", "6"], cwd=b, check=True,
                       capture_output=True, timeout=300, text=True)
    assert "Adaptive : rounds 3, tile-passes 576 of 576, tiles converged " in r.stdout
    assert (b / "result.png").read_bytes() == (a / "result.png").read_bytes()
    # a reachable target: the files are render_adaptive's arrays
    sc = _scene("cornell")
    cam, prm = ptamd.make_camera(W, H), prm_of(2, spp=2)
    ref = sc.render_adaptive(cam, prm, 0.0, 2)
    target = float(np.median(ref["tile_err"]))
    want = sc.render_adaptive(cam, prm, target, 8, min_passes=2)
    assert len(np.unique(want["tile_passes"])) >= 2
    r = subprocess.run(args + ["--passes", "2", "--adaptive", repr(target), "--max-passes", "8", "--pass-map", "p.bin", "--variance", "v.bin",
                               "--raw", "r.bin", "--denoise", "d.png"], cwd=c, check=True, capture_output=True, timeout=300, text=True)
    assert (c / "p.bin").read_bytes() == want["tile_passes"].tobytes()
    assert (c / "v.bin").read_bytes() == want["var"].tobytes() and (c / "r.bin").read_bytes() == want["rgb"].tobytes()
    assert (c / "result.png").stat().st_size > 0 and (c / "d.png").stat().st_size > 0
    rep = want["report"]
    assert f"Adaptive : rounds {rep['rounds']}, tile-passes {rep['tile_passes']} of {96 * 8}, tiles converged {rep['tiles_converged']} of 96" in r.stdout
    # without the new options the binary behaves as before: same output lines (but for the timings), same result.png
    again = subprocess.run(args + ["--passes", "6"], cwd=tmp_path, check=True, capture_output=True, timeout=300, text=True)
    assert (tmp_path / "result.png").read_bytes() == (a / "result.png").read_bytes()
    strip = lambda s: [ln for ln in s.splitlines() if "time" not in ln and "kernel_ms" not in ln]      # noqa: E731
    assert strip(again.stdout) == strip(plain.stdout)
    for extra in (["--target-error", "0.1"], ["--window", "0,0,8,8"], ["--views", "views.txt"]):
        bad = subprocess.run(args + ["--adaptive", "0.1"] + extra, cwd=tmp_path, capture_output=True, timeout=60, text=True)
        assert bad.returncode == 2 and "--adaptive" in bad.stderr, extra
    for extra in (["--min-passes", "4"], ["--pass-map", "p.bin"]):
        bad = subprocess.run(args + extra, cwd=tmp_path, capture_output=True, timeout=60, text=True)
        assert bad.returncode == 2, extra
