"""The a-trous denoiser (csrc/pt_denoise.hip: dn_pack, dn_atrous, dn_finish) bit for bit and pixel by pixel at its edges, on synthetic
frames of a few thousand pixels at the most.

The yardstick is denoise_ref.denoise32: the three kernels in float32, one rounding per operation, in the kernels' order.  The one
operation numpy cannot replay is the device's expf, so the EXACT FAMILY is built to make every exp argument -0.0: a random label in
{0, 1, 2} per pixel, the normal the label's unit axis (differing labels: |dn|^2 = 2, E >= 200 > 80 at sigma_normal 0.1), one depth
everywhere, sigma_color 3e19 (its square overflows: kc = 0, no colour term).  The weights are then the dyadic h products and the GPU
must return denoise32's bits.  Every reference of a bit-for-bit test is computed through a hook that asserts the premise: all exp
arguments are +-0.

CPU: the premise on every shape and L, denoise32 against the float64 definition, and six deliberately wrong restatements
(a switch in this module) that must change the bits.  GPU tests 1 - 7 are bits; test 8 (general inputs, the device's own expf) is per
pixel within 4 S, S the effect of moving every exp value by a seeded -1 / 0 / +1 ulp, computed from the reference alone."""
import numpy as np
import pytest

import denoise_ref as D
import ptamd
from scenes_util import test_spheres as make_test_spheres

F32 = np.float32
SHAPES = [(2, 2), (2, 17), (17, 2), (3, 5), (16, 16), (17, 33), (31, 47)]      # (H, W)
BIG = [s for s in SHAPES if s[0] * s[1] >= 15]
LS = (1, 2, 5, 12)
OFF = 3e19                               # sigma_color whose square overflows float32: kc = 0
T = D.THRESHOLD
T_UP, T_DOWN = np.nextafter(T, F32(1)), np.nextafter(T, F32(0))
GENERAL_SETS = (dict(), dict(sigma_color=0.5), dict(iterations=7))
RENDERED_SETS = ({}, dict(iterations=1), dict(iterations=2, demodulate=0, sigma_color=1.0),
                 dict(iterations=7, sigma_normal=0.5, sigma_depth=0.05, sigma_color=4.0), dict(iterations=12))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits_or_nan(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, want, what):
    ok = same_bits_or_nan(got, want)
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def exact_frame(H, W, seed, nonfinite=False):
    """A frame of the exact family; nonfinite: one NaN pixel, one +inf component, one -inf component and a 2 x 2 NaN block."""
    rs = np.random.RandomState(seed)
    aov = np.zeros((H, W, 8), F32)
    aov[..., 0:3] = rs.uniform(0.05, 1.0, (H, W, 3))
    aov[..., 3:6] = np.eye(3, dtype=F32)[rs.randint(0, 3, (H, W))]
    aov[..., 6] = 10.0
    aov[..., 7] = 1.0
    rgb = rs.uniform(0.0, 4.0, (H, W, 3)).astype(F32)
    if nonfinite:
        by, bx = rs.randint(0, H - 1), rs.randint(0, W - 1)
        rgb[by:by + 2, bx:bx + 2] = np.nan
        rest = [(y, x) for y in range(H) for x in range(W) if not (by <= y < by + 2 and bx <= x < bx + 2)]
        a, b, c = (rest[k] for k in rs.permutation(len(rest))[:3])
        rgb[a] = np.nan
        rgb[b][rs.randint(0, 3)] = np.inf
        rgb[c][rs.randint(0, 3)] = -np.inf
    return rgb, aov


def general_frame(H=37, W=45, seed=77):
    """Smooth normals, depth 10 + U(0, 1), random albedo and colour, a NaN pixel and an inf component: every exp argument matters."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    n = np.stack([0.3 * np.sin(x / 7.0), 0.3 * np.cos(y / 5.0), np.ones((H, W))], -1)
    aov = np.zeros((H, W, 8), F32)
    aov[..., 0:3] = rs.uniform(0.05, 1.0, (H, W, 3))
    aov[..., 3:6] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    aov[..., 6] = 10.0 + rs.uniform(0.0, 1.0, (H, W))
    aov[..., 7] = 1.0
    rgb = (rs.uniform(0.0, 4.0, (H, W, 3)) * aov[..., 0:3]).astype(F32)
    rgb[5, 7] = np.nan
    rgb[20, 30, 1] = np.inf
    return rgb, aov


class Recorder:
    """exp_fn hook: keeps every argument."""

    def __init__(self):
        self.args = []

    def __call__(self, x):
        self.args.append(np.array(x, F32))
        return D.exp32(x)


def exact32(rgb, aov, cnt, **kw):
    """denoise32, with the premise of a bit-for-bit comparison asserted: every exp argument is +-0."""
    rec = Recorder()
    out = D.denoise32(rgb, aov, cnt, exp_fn=rec, **kw)
    args = np.concatenate([a.ravel() for a in rec.args]) if rec.args else np.zeros(0, F32)
    assert (args == 0).all(), ("an exp argument is not 0", kw, np.unique(args)[:5])
    return out


def moved_exp(seed, k=1):
    """exp32 with every value moved by a seeded -k / 0 / +k ulp."""
    rs = np.random.RandomState(seed)

    def f(x):
        y = D.exp32(x)
        m = rs.randint(-1, 2, y.shape)
        for _ in range(k):
            y = np.where(m < 0, np.nextafter(y, F32(0)), np.where(m > 0, np.nextafter(y, F32(np.inf)), y)).astype(F32)
        return y
    return f


def rel_dev(a, ref, scale):
    """max |a - ref| over the pixels where ref is finite, over scale."""
    m = np.isfinite(ref)
    return float(np.abs(a.astype(np.float64)[m] - ref.astype(np.float64)[m]).max() / scale)


def exp_spread(rgb, aov, cnt, kw, ref32, scale, k=1):
    """S: the largest deviation from denoise32 that moving every exp value by -k / 0 / +k ulp causes, over 8 seeds, over scale."""
    return max(rel_dev(D.denoise32(rgb, aov, cnt, exp_fn=moved_exp(seed, k), **kw), ref32, scale) for seed in range(8))


# the restatement once more, compact, with a switch for the deliberately wrong variants (exact family only: every used weight is h h)
WRONG = ("last_column", "last_row", "step", "finite_flag", "stale_buffer", "h")


def filter32(rgb, aov, cnt, L, demodulate=1, wrong=None):
    H, W = rgb.shape[:2]
    h = F32([1 / 16, 1 / 4, 1 / 4 if wrong == "h" else 3 / 8, 1 / 4, 1 / 16])
    cnt = F32(cnt)
    kn = F32(1) / (F32(0.1) * F32(0.1))
    with np.errstate(all="ignore"):
        c = rgb / cnt
        div = np.where(aov[..., 0:3] > T, aov[..., 0:3], F32(1)) if demodulate else np.ones_like(c)
        cur = (c / div, np.isfinite(c).all(-1))
        before = cur
        n, z = aov[..., 3:6], aov[..., 6]
        for i in range(L):
            e, fin = before if (wrong == "stale_buffer" and i >= 2 and i % 2 == 0) else cur
            s = (1 << i) + (1 if wrong == "step" and i >= 1 else 0)
            acc, wsum = np.zeros_like(e), np.zeros((H, W), F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = np.arange(H) + s * dy, np.arange(W) + s * dx
                    vy = (qy >= 0) & (qy < (H - 1 if wrong == "last_row" else H))
                    vx = (qx >= 0) & (qx < (W - 1 if wrong == "last_column" else W))
                    g = np.ix_(np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1))
                    dn = n - n[g]
                    E = ((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]) * kn
                    mz = np.where(z > z[g], z, z[g])
                    E = np.where(mz > 0, E + np.abs(z - z[g]) * (F32(1) / F32(0.1)) / mz, E)
                    use = vy[:, None] & vx[None, :] & (E <= F32(80))
                    if wrong != "finite_flag":
                        use &= fin[g]
                    assert (E[use] == 0).all()
                    w = np.where(use, h[dx + 2] * h[dy + 2], F32(0))
                    acc = np.where(use[..., None], acc + w[..., None] * e[g], acc)
                    wsum = wsum + w
            o = acc / wsum[..., None]
            before = cur
            cur = (np.where((wsum > 0)[..., None], o, e), np.where(wsum > 0, np.isfinite(o).all(-1), fin))
        return (cur[0] * div) * cnt


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_family_premise(shape):
    """Every exp argument is +-0 on every shape, L, demodulate, with and without non-finite pixels (asserted inside exact32), and the
    filter is not the identity: it changes at least 90 % of the pixels of every frame of 15 pixels or more (measured: 93 - 100 %)."""
    H, W = shape
    least = 1.0
    for nonfinite in ((False, True) if H * W >= 15 else (False,)):
        rgb, aov = exact_frame(H, W, 100 + H * W, nonfinite)
        for L in LS:
            for dm in (0, 1):
                out = exact32(rgb, aov, 3, iterations=L, sigma_color=OFF, demodulate=dm)
                changed = float((~same_bits_or_nan(out, rgb).all(-1)).mean())
                least = min(least, changed)
                assert H * W < 15 or changed >= 0.90, (shape, L, dm, nonfinite, changed)
    print(f"{H}x{W}: at least {100 * least:.1f} % of the pixels changed")


def _against_float64(rgb, aov, cnt, kw):
    got = D.denoise32(rgb, aov, cnt, **kw)
    want = D.denoise(rgb, aov, cnt, **{**D.DEFAULTS, **kw})
    assert np.array_equal(np.isfinite(got), np.isfinite(want)), kw
    return rel_dev(got, want, np.abs(want[np.isfinite(want)]).max())


def test_denoise32_agrees_with_the_float64_definition():
    """Finite masks equal, max |diff| / max |want| <= 2e-6: four times the largest value measured when the restatement was written
    (4.5e-7; with these seeds 5.0e-8 - 1.8e-7 on the exact family, 3.9e-7 - 5.9e-7 on the general one)."""
    worst = 0.0
    for H, W in SHAPES:
        rgb, aov = exact_frame(H, W, 100 + H * W, H * W >= 15)
        for L in LS:
            r = _against_float64(rgb, aov, 3, dict(iterations=L, sigma_color=OFF))
            print(f"exact {H}x{W} L={L}: {r:.2e}")
            worst = max(worst, r)
    rgb, aov = general_frame()
    for kw in GENERAL_SETS:
        r = _against_float64(rgb, aov, 2, kw)
        print(f"general {kw}: {r:.2e}")
        worst = max(worst, r)
    assert worst <= 2e-6, worst


@pytest.mark.parametrize("shape", BIG)
def test_the_compact_restatement_is_denoise32(shape):
    rgb, aov = exact_frame(*shape, 100 + shape[0] * shape[1], True)
    for L in (1, 5):
        assert_same(filter32(rgb, aov, 3, L), exact32(rgb, aov, 3, iterations=L, sigma_color=OFF), (shape, L))


@pytest.mark.parametrize("wrong", WRONG)
@pytest.mark.parametrize("shape", BIG)
def test_a_wrong_filter_changes_the_bits(shape, wrong):
    """Sensitivity, numpy only: a tap bound off by one in x or y, step 2^i + 1 from i = 1 on, the tap's finite flag ignored, the
    ping-pong buffer not swapped before even iterations, h(0) = 1/4 — each changes the result of every frame of 15 pixels or more."""
    rgb, aov = exact_frame(*shape, 100 + shape[0] * shape[1], True)
    good = filter32(rgb, aov, 3, 5)
    assert not same_bits_or_nan(filter32(rgb, aov, 3, 5, wrong=wrong), good).all(), (shape, wrong)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    yield


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_family_bit_for_bit(_gpu, shape):
    """1: every shape x L x demodulate; frames of 15 pixels or more carry the non-finite pixels."""
    H, W = shape
    rgb, aov = exact_frame(H, W, 100 + H * W, H * W >= 15)
    for L in LS:
        for dm in (0, 1):
            kw = dict(iterations=L, sigma_color=OFF, demodulate=dm)
            assert_same(ptamd.denoise(rgb, aov, 3, **kw), exact32(rgb, aov, 3, **kw), (shape, kw))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(17, 33), (3, 5)])
def test_batch_bit_for_bit(_gpu, shape):
    """2: three different frames of an odd pixel count, stacked: a tap that crossed a frame boundary would show."""
    H, W = shape
    frames = [exact_frame(H, W, 300 + k, True) for k in range(3)]
    rgb, aov = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    for L in (3, 12):
        kw = dict(iterations=L, sigma_color=OFF)
        got = ptamd.denoise_batch(rgb, aov, 2, **kw)
        for k in range(3):
            assert_same(got[k], exact32(rgb[k], aov[k], 2, **kw), (shape, L, k))


@pytest.mark.gpu
def test_device_pointers_unaligned_frame(_gpu):
    """3: pt_denoise with d_rgb and d_out 4 bytes past a 16-byte boundary (only d_aov and d_work must be aligned); nothing is written
    outside the frame."""
    import torch
    H, W = 17, 33
    n = H * W
    rgb, aov = exact_frame(H, W, 100 + n, True)
    dev = torch.device("cuda:0")
    d_rgb = torch.zeros(3 * n + 8, dtype=torch.float32, device=dev)
    d_out = torch.full((3 * n + 8,), -7.0, dtype=torch.float32, device=dev)
    d_aov = torch.from_numpy(aov).to(dev)
    d_work = torch.empty(ptamd.denoise_work_bytes(W, H), dtype=torch.uint8, device=dev)
    d_rgb[1:1 + 3 * n] = torch.from_numpy(rgb.ravel()).to(dev)
    assert d_rgb.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0 and d_aov.data_ptr() % 16 == 0 and d_work.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    kw = dict(iterations=5, sigma_color=OFF)
    ptamd.denoise_device(d_rgb.data_ptr() + 4, d_aov.data_ptr(), W, H, 3, d_out.data_ptr() + 4, d_work.data_ptr(), 0, **kw)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert out[0] == -7.0 and (out[1 + 3 * n:] == -7.0).all()
    assert_same(out[1:1 + 3 * n].reshape(H, W, 3), exact32(rgb, aov, 3, **kw), "device pointers")


def _threshold_candidates(rgb_px, div, cnt):
    """out of a pixel whose one usable tap is itself, L = 1: ((w (c / div)) / w) div cnt, w = h(0) h(0)."""
    w = F32(3 / 8) * F32(3 / 8)
    return (((w * ((rgb_px / F32(cnt)) / div)) / w) * div) * F32(cnt)


@pytest.mark.gpu
def test_albedo_threshold(_gpu):
    """4: albedo == float32(1e-3) and below divide by 1, the next float above divides by itself."""
    rgb, aov = exact_frame(4, 4, 41)
    aov[0, 1, 0:3] = (T, T_UP, T_DOWN)
    aov[1, 1, 0:3] = (0.0, T, T_UP)
    aov[2, 2, 0:3] = (T_DOWN, 0.0, T)
    aov[3, 0, 0:3] = T
    aov[1, 3, 0:3] = T_UP
    for L in (1, 2):
        kw = dict(iterations=L, sigma_color=OFF)
        assert_same(ptamd.denoise(rgb, aov, 3, **kw), exact32(rgb, aov, 3, **kw), L)
    # directly: three pixels with normals of their own (no other usable tap), L = 1
    rgb, aov = exact_frame(4, 4, 42)
    where = {(0, 0): T, (1, 2): T_DOWN, (3, 1): T_UP}
    rs = np.random.RandomState(43)
    for k, (p, a) in enumerate(where.items()):
        aov[p][0:3] = a
        aov[p][3:6] = -np.eye(3, dtype=F32)[k]
        # a colour on which dividing by 1 and dividing by the albedo round differently in every channel, so that the result tells which was done
        while (bits(_threshold_candidates(rgb[p], F32(1), 3)) == bits(_threshold_candidates(rgb[p], a, 3))).any():
            rgb[p] = rs.uniform(0.0, 4.0, 3)
    kw = dict(iterations=1, sigma_color=OFF)
    got = ptamd.denoise(rgb, aov, 3, **kw)
    assert_same(got, exact32(rgb, aov, 3, **kw), "direct")
    for p, a in where.items():
        by_one, by_albedo = _threshold_candidates(rgb[p], F32(1), 3), _threshold_candidates(rgb[p], a, 3)
        assert (bits(by_one) != bits(by_albedo)).any(), "the two readings must differ on this pixel for the assertion to say anything"
        assert np.array_equal(bits(got[p]), bits(by_albedo if a == T_UP else by_one)), (p, a)


def _cutoff_frame(ny):
    rgb = np.ones((2, 2, 3), F32)
    rgb[0, 0] = np.nan
    aov = np.zeros((2, 2, 8), F32)
    aov[..., 0:3] = 0.5
    aov[..., 6] = 10.0
    aov[..., 7] = 1.0
    aov[0, 1, 3:6] = (1.0, ny, 0.0)                      # |dn|^2 = 1 + ny^2 against the NaN pixel's normal 0
    aov[1, 0, 3:6] = (0.0, 0.0, 10.0)
    aov[1, 1, 3:6] = (0.0, 10.0, 0.0)
    return rgb, aov


@pytest.mark.gpu
def test_cutoff_is_inclusive(_gpu):
    """5: sigma_normal 0.25 (kn = 16 exactly), a neighbour at |dn|^2 = 5: E = 80 exactly is used and heals the NaN pixel; with the next
    float above 2 in the normal, E = 80.000008 is not."""
    kw = dict(iterations=1, sigma_normal=0.25, sigma_color=OFF)
    above = np.nextafter(F32(2), F32(3))
    assert (F32(1) + F32(2) * F32(2)) * F32(16) == F32(80) and (F32(1) + above * above) * F32(16) > F32(80)
    for ny, healed in ((2.0, True), (above, False)):
        got = ptamd.denoise(*_cutoff_frame(ny), 1, **kw)
        assert np.isfinite(got[[0, 1, 1], [1, 0, 1]]).all()
        assert np.isfinite(got[0, 0]).all() if healed else np.isnan(got[0, 0]).all(), (ny, got[0, 0])
        assert np.array_equal(np.isfinite(got), np.isfinite(D.denoise32(*_cutoff_frame(ny), 1, **kw))), ny


def _odd_frame(colour=None):
    rgb, aov = exact_frame(9, 11, 61)
    aov[4, 5, 3:6] = np.nan                              # a zero-area triangle's normal
    aov[1, 2, 6] = np.inf
    aov[6:9, 0:4, 6] = -5.0                              # a region of negative depth
    aov[0:3, 7:11, 6] = 0.0                              # a miss region: no albedo, no normal, depth 0, coverage 0
    aov[0:3, 7:11, 0:6] = 0.0
    aov[0:3, 7:11, 7] = 0.0
    aov[7, 8, 6] = np.nan
    if colour is not None:
        rgb[4, 5] = colour
    return rgb, aov


@pytest.mark.gpu
def test_odd_features(_gpu):
    """6: a NaN normal, depths +inf, NaN, -5 among -5 and 0 among 0.  sigma_depth 0.01 keeps the regions' borders above the cutoff
    (|0 - 10| 100 / 10 = 100, |-5 - 10| 100 / 10 = 150), so the frame is still of the exact family."""
    rgb, aov = _odd_frame()
    rgb2, _ = _odd_frame(colour=(9.0, 0.25, 3.0))
    cnt = 3
    for L in (1, 3):
        kw = dict(iterations=L, sigma_color=OFF, sigma_depth=0.01)
        got, got2 = ptamd.denoise(rgb, aov, cnt, **kw), ptamd.denoise(rgb2, aov, cnt, **kw)
        assert_same(got, exact32(rgb, aov, cnt, **kw), L)
        assert_same(got2, exact32(rgb2, aov, cnt, **kw), L)
        # the pixel with the NaN normal, and the one at depth +inf, keep their value ...
        for frame, out in ((rgb, got), (rgb2, got2)):
            for p in ((4, 5), (1, 2)):
                div = aov[p][0:3]
                assert (div > T).all()
                assert np.array_equal(bits(out[p]), bits((((frame[p] / F32(cnt)) / div) * div) * F32(cnt))), (L, p)
        # ... and the NaN-normal pixel is nobody's tap: its colour reaches no other pixel
        other = np.ones((9, 11), bool)
        other[4, 5] = False
        assert np.array_equal(bits(got)[other], bits(got2)[other]) and not np.array_equal(bits(got[4, 5]), bits(got2[4, 5]))
        # a pair with max depth <= 0 has no depth term: the regions of depth -5 and 0 are filtered among themselves
        assert (bits(got[6:9, 0:4]) != bits(rgb[6:9, 0:4])).any(-1).mean() >= 0.75
        assert (bits(got[0:3, 7:11]) != bits(rgb[0:3, 7:11])).any(-1).all()


@pytest.mark.gpu
def test_parameter_corners(_gpu):
    """7: sigma_color 1e-19 (kc = 1e38, inf from the second iteration on: the centre tap's 0 * inf is NaN and every pixel is kept, so
    L = 3 is L = 1), sample_cnt 1, 2^24 + 1 (no float32) and 2^31 - 1, and two depth regions under sigma_depth 0.005 (E = 150)."""
    H, W = 17, 33
    rgb, aov = exact_frame(H, W, 100 + H * W, True)
    got3 = ptamd.denoise(rgb, aov, 3, iterations=3, sigma_color=1e-19)
    assert_same(got3, exact32(rgb, aov, 3, iterations=3, sigma_color=1e-19), "sigma_color 1e-19")
    assert_same(got3, ptamd.denoise(rgb, aov, 3, iterations=1, sigma_color=1e-19), "L = 3 against L = 1")
    assert_same(ptamd.denoise(rgb, aov, 3, iterations=3, sigma_color=1e-30), exact32(rgb, aov, 3, iterations=3, sigma_color=1e-30),
                "sigma_color 1e-30: its square is 0")
    for cnt in (1, 2 ** 24 + 1, 2 ** 31 - 1):
        kw = dict(iterations=5, sigma_color=OFF)
        assert_same(ptamd.denoise(rgb, aov, cnt, **kw), exact32(rgb, aov, cnt, **kw), cnt)
    aov[:, 20:, 6] = 40.0
    aov[9:, :6, 6] = 40.0
    kw = dict(iterations=5, sigma_color=OFF, sigma_depth=0.005)
    assert_same(ptamd.denoise(rgb, aov, 3, **kw), exact32(rgb, aov, 3, **kw), "two depth regions")


@pytest.fixture(scope="module")
def rendered(_gpu):
    """The frame of test_denoise.test_denoiser_matches_its_definition: standin_spheres, 100 x 52, with its NaN and inf pixels."""
    sc = ptamd.Scene.from_prims(ptamd.gen_scene(1, 16), make_test_spheres())
    W, H, passes = 100, 52, 2
    cam = ptamd.make_camera(W, H)
    rgb = sc.render(cam, ptamd.default_params(passes=passes, spp_per_pass=2, max_bounce=12))
    aov, _ = sc.aov(cam, ptamd.default_params(passes=passes))
    rgb[10, 10] = np.nan
    rgb[0, 0] = np.nan
    rgb[20, 30, 1] = np.inf
    rgb[30, 50, 2] = -np.inf
    rgb[H - 1, W - 1, 0] = np.nan
    rgb[40:46, 70:76] = np.nan
    return rgb, aov, passes


def _per_pixel(rgb, aov, cnt, kw, what):
    got = ptamd.denoise(rgb, aov, cnt, **kw)
    ref = D.denoise32(rgb, aov, cnt, **kw)
    want = D.denoise(rgb, aov, cnt, **{**D.DEFAULTS, **kw})
    assert np.array_equal(np.isfinite(got), np.isfinite(ref)) and np.array_equal(np.isfinite(ref), np.isfinite(want)), (what, kw)
    scale = np.abs(want[np.isfinite(want)]).max()
    S = exp_spread(rgb, aov, cnt, kw, ref, scale)
    dev = rel_dev(got, ref, scale)
    print(f"{what} {kw}: S {S:.2e}, GPU - denoise32 {dev:.2e} = {dev / S:.2f} S, denoise32 - float64 {rel_dev(ref, want, scale):.2e}, "
          f"pixels with other bits {100 * float((~same_bits_or_nan(got, ref).all(-1)).mean()):.1f} %")
    assert dev <= 4 * S, (what, kw, dev, S)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(GENERAL_SETS)))
def test_general_frame_per_pixel(_gpu, k):
    """8a: the synthetic general frame, every finite pixel within 4 S of denoise32.  Measured on an MI355X: S 3.7e-7 - 4.6e-7, the GPU
    0.50 - 0.67 S away, 5 - 34 % of the pixels with other bits than denoise32."""
    rgb, aov = general_frame()
    _per_pixel(rgb, aov, 2, GENERAL_SETS[k], "general")


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(RENDERED_SETS)))
def test_rendered_frame_per_pixel(rendered, k):
    """8b: the rendered frame and the five parameter sets of test_denoiser_matches_its_definition, every finite pixel within 4 S.
    Measured on an MI355X: S 1.4e-7 - 2.1e-7, the GPU 0.50 - 0.67 S away."""
    rgb, aov, passes = rendered
    _per_pixel(rgb, aov, passes, RENDERED_SETS[k], "rendered")
