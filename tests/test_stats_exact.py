"""The moments and error-estimate kernels of csrc/pt_stats.hip on every path, bit for bit, on synthetic buffers (no render: the start of
d_work IS the staging slab, so a test hands the calls a pass-major slab of its own).

CPU: estimate32 (stats_ref.py, the kernel's own summation order) against the float64 definition under a derived bound; deliberately wrong
variants of the fold, the variance and the estimate each change the bits on the inputs the GPU tests use; misaligned buffers are refused
before any HIP call.  GPU: pt_accumulate_passes (float4 and scalar kernel) against R.fold, pt_variance (both kernels) against R.variance,
pt_error_estimate (VEC and not, one and two grid-stride trips, every rank) against estimate32, the list calls against adaptive_ref with
entries outside the frame, pt_finish_tiles at n = 0, 1 and where (float)n rounds.  A NaN equals a NaN (its payload is the hardware's)."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref as A
import stats_ref as R
import ptamd
from test_stats import bits

F = np.float32
SENTINEL = 0x7FC12345                    # a NaN pattern no computation here produces: guards around every device buffer
GUARD = 4                                # int32 words of it on either side (16 bytes: the payload's alignment is the offset's)
FOLD_FRAMES = ((8, 8), (64, 48), (100, 52))      # one tile; whole tiles; ragged on both edges (91 tiles: world 2 and 3 leave a tile over)
WORLDS = (1, 2, 3)
PASSES = (1, 2, 3, 17)
N_BEFORE = (0, 5, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, "max")      # (float)k rounds from 2^24 + 1 on; max = what the argument check allows
KINDS = ("render", "near", "negative", "tiny", "huge", "special")
VAR_FLOATS = (1, 2, 3, 5, 191, 192, 193)
VAR_PASSES = (2, 3, 2 ** 24 + 1, 2 ** 31 - 1)
EST_N = 5                                # 0.03f * 5 is not exact in float32
EST_SMALL = [(W, H, rank, world) for W, H in ((100, 52), (64, 48)) for world in WORLDS for rank in range(world)]
EST_BIG = [(1025, 1023, 0, 1), (2049, 1023, 0, 2), (2049, 1023, 1, 2)]      # 16,512 tiles: a ragged second trip; 16,448 local: over the cap
ids4 = lambda c: f"{c[0]}x{c[1]}-rank{c[2]}of{c[3]}"      # noqa: E731


def same(got, want):
    """Same bits, or NaN on both sides."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    return got.shape == want.shape and bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def n_before_of(nb, passes):
    return 2 ** 31 - 1 - passes if nb == "max" else nb


# ---------------------------------------------------------------------------------------------------------------------------------
# the inputs, shared by the CPU sensitivity tests and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
def fold_slab(passes, n, seed=1):
    """(passes, n) float32 pass means; float i is of kind KINDS[i % 6], so every kind meets every lane of a float4."""
    rs = np.random.RandomState(seed)
    x = np.empty((passes, n), F)
    k = np.arange(n) % len(KINDS)
    x[:, k == 0] = (4 * rs.uniform(0, 1, (passes, (k == 0).sum())) ** 4).astype(F)
    x[:, k == 1] = (15.01 + 1e-4 * rs.standard_normal((passes, (k == 1).sum()))).astype(F)
    x[:, k == 2] = (-3 * rs.uniform(0, 1, (passes, (k == 2).sum()))).astype(F)
    x[:, k == 3] = rs.choice(np.array([1e-40, -1e-40, 1.4e-45, -1.4e-45, 3e-39, 7e-39], F), (passes, (k == 3).sum()))
    x[:, k == 4] = F(3e38)
    sp = (2 * rs.uniform(0, 1, (passes, (k == 5).sum())) ** 2).astype(F)
    pick = rs.randint(0, 12, sp.shape)
    for code, v in enumerate((np.inf, -np.inf, np.nan, -0.0)):
        sp[pick == code] = F(v)
    x[:, k == 5] = sp
    return x


def fold_state(n, n_before, seed=2):
    """A state (S, M2) to fold into; every 11th float of S and every 13th of M2 is NaN.  n_before = 0: all NaN, and never read."""
    if n_before == 0:
        return np.full(n, np.nan, F), np.full(n, np.nan, F)
    rs = np.random.RandomState(seed)
    mean = fold_slab(1, n, seed + 7)[0]
    mean[~np.isfinite(mean)] = F(1.5)
    with np.errstate(over="ignore"):
        S = (mean * F(n_before)).astype(F)
    M2 = (rs.uniform(0, 1, n) ** 2 * min(n_before, 1000)).astype(F)
    M2[(np.arange(n) % len(KINDS)) == 3] = F(2e-40)
    S[::11] = np.nan
    M2[::13] = np.nan
    return S, M2


VAR_POOL = np.concatenate([np.array([2.0 ** 100, np.nan, -1e-9, -0.0, np.inf, 1e-40, -np.inf, 0.0, 3.0, -2.0 ** 100, 1.4e-45, 3e38], F),
                           (np.random.RandomState(9).uniform(0, 1, 193) ** 3 * 50).astype(F)])


def var_input(n_floats, shift=0):
    return VAR_POOL[(np.arange(n_floats) + shift) % VAR_POOL.size].copy()


def est_slab(W, H, rank, world, n=EST_N, seed=3, pad=0.0):
    """Tile-layout moments (S, M2) of rank's tiles, n_tiles_local * 192 floats each: render-like values, and at fixed strides of pixels a
    NaN or -inf S, an inf or NaN M2 beside a finite S, a negative M2, a negative S, subnormals; `pad` in every float outside the frame."""
    npx = R.tiles_local(W, H, world) * 64
    rs = np.random.RandomState(seed + 10 * rank)
    S = (n * 2 * rs.uniform(0, 1, (npx, 3)) ** 4).astype(F)
    M2 = (n * 0.5 * rs.uniform(0, 1, (npx, 3)) ** 6).astype(F)
    i = np.arange(npx)
    S[i % 97 == 5, 1] = np.nan
    S[i % 103 == 17, 0] = -np.inf
    M2[i % 89 == 7, 2] = np.inf
    M2[i % 101 == 13, 1] = np.nan
    M2[i % 83 == 3, 0] = F(-1e-3)
    S[i % 79 == 11] *= F(-1)
    S[i % 107 == 19] = F(1e-40)
    M2[i % 107 == 19] = F(1e-42)
    out = ~R.in_frame(W, H, rank, world)
    S[out], M2[out] = F(pad), F(pad)
    return S.reshape(-1), M2.reshape(-1)


def order_frame():
    """64 x 56, n = 2 (Var = 2 M2): 56 tiles, 4 blocks of 256 threads x 4 pixels, one trip.  Var 2^60 in wave 0 of block 0 and Var ~ 153.6
    (0.6 ulp of 2^60 in float64) in waves 1 - 3 of block 0 and in blocks 1 - 3; S = 1 everywhere.  Which of the small terms round up
    depends on the order they meet the large one in: the wave order and the block order both show in rel_rms."""
    W, H = 64, 56
    S, M2 = np.ones((56 * 64, 3), F), np.zeros((56 * 64, 3), F)
    M2[0, 0] = F(2.0 ** 59)
    for wave in (1, 2, 3):
        M2[4 * 64 * wave, 1] = F(76.8)          # thread 64 w of block 0: group 64 w, pixel 256 w
    for block in (1, 2, 3):
        M2[4 * 256 * block, 2] = F(76.8)        # thread 0 of block b: group 256 b
    return W, H, S.reshape(-1), M2.reshape(-1)


def from_tiles(t, W, H):
    """(tiles * 192,) frame tile layout -> (H, W, 3)"""
    ty, tx = A.tile_grid(W, H)
    return np.asarray(t).reshape(ty, tx, 8, 8, 3).transpose(0, 2, 1, 3, 4).reshape(ty * 8, tx * 8, 3)[:H, :W]


def est_key(e):
    return (np.float64(e["rel_rms"]).view(np.uint64).item(), np.float64(e["mean_rel_se"]).view(np.uint64).item(), e["pixels"], e["skipped"])


def same_estimate(got, want):
    """The four fields; a float64 field matches by its bits, or when both are NaN."""
    return (got["pixels"], got["skipped"]) == (want["pixels"], want["skipped"]) and all(
        np.float64(got[k]).view(np.uint64) == np.float64(want[k]).view(np.uint64) or (np.isnan(got[k]) and np.isnan(want[k]))
        for k in ("rel_rms", "mean_rel_se"))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: estimate32 against the float64 definition
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EST_SMALL + EST_BIG[:1], ids=ids4)
def test_estimate32_agrees_with_the_float64_definition(case):
    W, H, rank, world = case
    S, M2 = est_slab(W, H, rank, world)
    got = R.estimate32(S, M2, EST_N, W, H, rank, world)
    here = R.in_frame(W, H, rank, world)
    want = R.estimate(S.reshape(-1, 3)[here], M2.reshape(-1, 3)[here], EST_N)
    bound = R.summation_bound(S.size, want["pixels"])
    dev = {k: abs(got[k] - want[k]) / want[k] for k in ("rel_rms", "mean_rel_se")}
    print(f"{ids4(case)}: estimate32 vs float64 definition rel_rms {dev['rel_rms']:.2e}, mean_rel_se {dev['mean_rel_se']:.2e}, bound {bound:.2e}; {got}")
    assert (got["pixels"], got["skipped"]) == (want["pixels"], want["skipped"]) and got["skipped"] > 0
    assert got["pixels"] + got["skipped"] == int(here.sum())
    assert dev["rel_rms"] <= bound and dev["mean_rel_se"] <= bound


def test_estimate32_degenerate_frames():
    """All S = M2 = 0: 0 / 0 under the root, every term 0 / (0.03 n).  Every pixel skipped: 0 / 0 in both."""
    W, H = 20, 12
    z = np.zeros(R.tiles_local(W, H, 1) * 192, F)
    e = R.estimate32(z, z, 4, W, H)
    assert np.isnan(e["rel_rms"]) and e["mean_rel_se"] == 0.0 and (e["pixels"], e["skipped"]) == (W * H, 0)
    e = R.estimate32(np.full_like(z, np.nan), z, 4, W, H)
    assert np.isnan(e["rel_rms"]) and np.isnan(e["mean_rel_se"]) and (e["pixels"], e["skipped"]) == (0, W * H)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: a wrong kernel would change the bits on the inputs the GPU tests use
# ---------------------------------------------------------------------------------------------------------------------------------
FOLD_WRONG = ("d2_from_s_prev", "reciprocal", "contracted", "flushed")
# the kinds of fold_slab that must show each variant (the test prints all that do)
FOLD_CATCHERS = {"d2_from_s_prev": ("render", "near", "negative"), "reciprocal": ("render", "negative"), "contracted": ("render", "negative"),
                 "flushed": ("tiny",)}


def _ftz(x):
    return np.where(np.abs(x) < F(2.0 ** -126), np.copysign(F(0), x), x).astype(F)


def fold_variant(means, S, M2, n_before, wrong=None):
    """R.fold written out again with one switch: d2 from S_prev; S / k as S * (1 / k); M2 + d1 d2 with one rounding (from float64: the
    product of two float32 is exact there); subnormal inputs and results flushed to zero."""
    z = _ftz if wrong == "flushed" else (lambda x: x)
    if n_before == 0:
        S, M2 = np.zeros(means.shape[1:], F), np.zeros(means.shape[1:], F)
    S, M2 = z(np.array(S, F)), z(np.array(M2, F))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for j in range(means.shape[0]):
            k = n_before + j + 1
            m, Sp = z(means[j]), S
            S = z(Sp + m)
            if k >= 2:
                d1 = z(m - z(Sp / F(k - 1)))
                if wrong == "d2_from_s_prev":
                    d2 = m - Sp / F(k)
                elif wrong == "reciprocal":
                    d2 = m - S * (F(1) / F(k))
                else:
                    d2 = z(m - z(S / F(k)))
                if wrong == "contracted":
                    M2 = (M2.astype(np.float64) + d1.astype(np.float64) * d2.astype(np.float64)).astype(F)
                else:
                    M2 = z(M2 + z(d1 * d2))
    assert S.dtype == F and M2.dtype == F
    return S, M2


def _fold_cases(n):
    for passes in PASSES:
        slab = fold_slab(passes, n)
        for nb in N_BEFORE:
            nb = n_before_of(nb, passes)
            yield slab, fold_state(n, nb), nb


def test_fold_variant_without_a_switch_is_the_fold():
    for slab, (S0, M0), nb in _fold_cases(192 * 3):
        a, b = fold_variant(slab, S0, M0, nb), R.fold(slab, S0, M0, nb)
        assert same(a[0], b[0]) and same(a[1], b[1]), (slab.shape[0], nb)


@pytest.mark.parametrize("wrong", FOLD_WRONG)
def test_a_wrong_fold_changes_the_bits(wrong):
    caught = set()
    for slab, (S0, M0), nb in _fold_cases(192 * 3):
        a, b = fold_variant(slab, S0, M0, nb, wrong), R.fold(slab, S0, M0, nb)
        diff = ~((bits(a[0]) == bits(b[0])) | (np.isnan(a[0]) & np.isnan(b[0]))) | ~((bits(a[1]) == bits(b[1])) | (np.isnan(a[1]) & np.isnan(b[1])))
        caught |= {KINDS[i] for i in np.unique(np.flatnonzero(diff) % len(KINDS))}
    print(f"fold variant {wrong}: shown by {sorted(caught)}")
    assert set(FOLD_CATCHERS[wrong]) <= caught, (wrong, caught)


VAR_WRONG = {
    "fmaxf": (lambda m, n: (np.fmax(m, F(0)) * F(n)) / F(n - 1)),                          # drops the NaN
    "ratio_first": (lambda m, n: np.where(m < 0, F(0), m) * (F(n) / F(n - 1))),            # M2 * (n / (n - 1)): no overflow at 2^31 - 1
    "nf_minus_one": (lambda m, n: (np.where(m < 0, F(0), m) * F(n)) / (F(n) - F(1))),      # (float)n - 1 for (float)(n - 1): 2^24 + 1
}
VAR_CATCHERS = {"fmaxf": VAR_PASSES, "ratio_first": (2 ** 31 - 1,), "nf_minus_one": (2 ** 24 + 1,)}


@pytest.mark.parametrize("wrong", list(VAR_WRONG))
def test_a_wrong_variance_changes_the_bits(wrong):
    caught = set()
    with np.errstate(invalid="ignore", over="ignore"):
        for n in VAR_PASSES:
            m = var_input(193)
            got = VAR_WRONG[wrong](m, n)
            assert got.dtype == F
            if not same(got, R.variance(m, n)):
                caught.add(n)
    print(f"variance variant {wrong}: shown at n_passes {sorted(caught)}")
    assert set(VAR_CATCHERS[wrong]) <= caught, (wrong, caught)
    v = R.variance(F([2.0 ** 100]), 2 ** 31 - 1)
    assert np.isinf(v[0])                      # (2^100 * 2^31) / 2^31: the product overflows, as the written order demands


EST_CATCHERS = {      # wrong variant -> the case of the GPU test that shows it: (W, H, rank, world, pad) or "order"
    "one_trip": (1025, 1023, 0, 1, 0.0), "rank_ignored": (100, 52, 1, 2, 0.0), "padding_counted": (100, 52, 0, 1, 1e30),
    "channels_in_float32": (100, 52, 0, 1, 0.0), "finite_s_only": (100, 52, 0, 1, 0.0), "bias_in_float64": (100, 52, 0, 1, 0.0),
    "waves_reversed": "order", "blocks_reversed": "order",
}


@pytest.mark.parametrize("wrong", R.EST_WRONG)
def test_a_wrong_estimate_changes_the_bits(wrong):
    case = EST_CATCHERS[wrong]
    if case == "order":
        W, H, S, M2 = order_frame()
        n, rank, world = 2, 0, 1
    else:
        W, H, rank, world, pad = case
        n = EST_N
        S, M2 = est_slab(W, H, rank, world, pad=pad)
    right, got = R.estimate32(S, M2, n, W, H, rank, world), R.estimate32(S, M2, n, W, H, rank, world, wrong=wrong)
    print(f"estimate variant {wrong}: {right} -> {got}")
    assert est_key(got) != est_key(right)
    if case == "order":
        assert got["rel_rms"] != right["rel_rms"] and (got["pixels"], got["skipped"]) == (W * H, 0)


def test_random_frames_do_not_show_the_wave_or_block_order():
    """Why order_frame exists: on the random frames the two reversals leave every bit as it is (float64 sums of float32 terms of like size)."""
    hidden = 0
    for W, H, rank, world in EST_SMALL:
        S, M2 = est_slab(W, H, rank, world)
        right = est_key(R.estimate32(S, M2, EST_N, W, H, rank, world))
        hidden += all(est_key(R.estimate32(S, M2, EST_N, W, H, rank, world, wrong=w)) == right for w in ("waves_reversed", "blocks_reversed"))
    print(f"reversed waves and blocks leave the bits alone on {hidden} of {len(EST_SMALL)} random frames")
    assert hidden >= len(EST_SMALL) // 2


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: alignment is checked before any device call
# ---------------------------------------------------------------------------------------------------------------------------------
def test_misaligned_buffers_are_rejected_before_any_device_call():
    """Fake device addresses, never dereferenced: float and int32 buffers need 4 bytes, d_scratch and d_err 8, the float4 buffers of the
    list calls 16.  The same calls with aligned fake addresses are NOT made: they would reach the device."""
    l = ptamd.lib()
    W, H = 16, 8
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=2)
    bc, bp = C.byref(cam), C.byref(prm)
    base = 1 << 40
    A_ = [base + (i << 20) for i in range(8)]
    out = ptamd.PtErrorEstimate()

    def each(call, args, where, offsets):
        """every pointer argument in `where`, moved by every offset: PT_ERR_INVALID and a message that names the call"""
        for at in where:
            for off in offsets[at] if isinstance(offsets, dict) else offsets:
                a = list(args)
                a[at] = a[at] + off
                a = [C.c_void_p(v) if isinstance(v, int) and v >= base else v for v in a]
                assert getattr(l, call)(*a, None) == -1, (call, at, off)
                assert call in l.pt_last_error().decode() and "aligned" in l.pt_last_error().decode(), (call, at, off)

    odd = (1, 2, 3)
    each("pt_accumulate_passes", (A_[0], bc, bp, 0, A_[1], A_[2]), (0, 4, 5), odd)
    each("pt_variance", (A_[0], 192, 2, A_[1]), (0, 3), odd)
    each("pt_error_estimate", (A_[0], A_[1], bc, bp, 2, A_[2], C.byref(out)), (0, 1, 5), {0: odd, 1: odd, 5: odd + (4, 12)})
    quad = odd + (4, 8, 12)
    each("pt_accumulate_tile_list", (A_[0], bc, bp, A_[1], 2, 0, A_[2], A_[3], A_[4]), (0, 3, 6, 7, 8), {0: quad, 6: quad, 7: quad, 3: odd, 8: odd})
    each("pt_tile_errors", (A_[0], A_[1], bc, A_[2], 2, 2, A_[3]), (0, 1, 3, 6), {0: odd, 1: odd, 3: odd, 6: odd + (4, 12)})
    each("pt_finish_tiles", (A_[0], A_[1], A_[2], bc, A_[3], A_[4]), (0, 1, 2, 4, 5), {0: quad, 1: quad, 2: odd, 4: quad, 5: quad})
    each("pt_finish_tiles", (A_[0], A_[1], A_[2], bc, None, A_[4]), (5,), quad)      # a NULL output beside a misaligned one
    each("pt_finish_tiles", (A_[0], A_[1], A_[2], bc, A_[3], None), (4,), quad)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    yield


class Buf:
    """A device buffer holding the 32-bit words of `a`, `off` words past a 16-byte boundary, between guards.  Everything here runs on the
    NULL stream, which is torch's default stream: the calls below and torch's copies are in order."""

    def __init__(self, a, off=0):
        import torch
        w = np.ascontiguousarray(a).reshape(-1).view(np.int32)
        self.n, self.lo = w.size, GUARD + off
        self.t = torch.full((self.lo + self.n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
        self.t[self.lo:self.lo + self.n] = torch.from_numpy(w.copy()).to("cuda:0")
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + 4 * self.lo

    def get(self, dtype=F):
        h = self.t.cpu().numpy()
        assert (h[:self.lo] == SENTINEL).all() and (h[self.lo + self.n:] == SENTINEL).all(), "written outside the buffer"
        return h[self.lo:self.lo + self.n].view(dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("size", FOLD_FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fold_bit_for_bit(_gpu, size, world):
    W, H = size
    cam = ptamd.make_camera(W, H)
    for passes in PASSES:
        prm = ptamd.default_params(passes=passes, rank=world - 1, world=world)
        n = ptamd.tiles_floats(cam, prm)
        assert n == R.tiles_local(W, H, world) * 192
        slab = fold_slab(passes, n)
        work = Buf(slab)
        for nb in N_BEFORE:
            nb = n_before_of(nb, passes)
            S0, M0 = fold_state(n, nb)
            dS, dM = Buf(S0), Buf(M0)
            ptamd.accumulate_passes(work.ptr, cam, prm, nb, dS.ptr, dM.ptr)
            wS, wM = R.fold(slab, S0, M0, nb)
            gS, gM = dS.get(), dM.get()
            assert same(gS, wS), (size, world, passes, nb, np.flatnonzero(bits(gS) != bits(wS))[:6])
            assert same(gM, wM), (size, world, passes, nb, np.flatnonzero(bits(gM) != bits(wM))[:6])
            if nb == 0 and passes == 2:      # S overflowed where it should, and a sum of subnormals is one
                assert np.isinf(gS[4]) and ((bits(gS[3::6]) & 0x7F800000 == 0) & (bits(gS[3::6]) & 0x007FFFFF != 0)).any()
        assert np.array_equal(bits(work.get()), bits(slab).reshape(-1))      # the slab is only read


@pytest.mark.gpu
@pytest.mark.parametrize("n_before", (0, 5))
def test_fold_scalar_kernel_bit_for_bit(_gpu, n_before):
    """Each buffer in turn 4, 8 and 12 bytes past a 16-byte boundary: st_fold<float>, the bits of the float4 path and of R.fold."""
    W, H, passes = 100, 52, 3
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=passes)
    n = ptamd.tiles_floats(cam, prm)
    slab = fold_slab(passes, n)
    S0, M0 = fold_state(n, n_before)
    wS, wM = R.fold(slab, S0, M0, n_before)
    for which in range(3):
        for off in (1, 2, 3):
            o = [off if which == b else 0 for b in range(3)]
            work, dS, dM = Buf(slab, o[0]), Buf(S0, o[1]), Buf(M0, o[2])
            assert work.ptr % 16 == 4 * o[0] and dS.ptr % 16 == 4 * o[1] and dM.ptr % 16 == 4 * o[2]
            ptamd.accumulate_passes(work.ptr, cam, prm, n_before, dS.ptr, dM.ptr)
            assert same(dS.get(), wS) and same(dM.get(), wM), (which, off)
            work.get()


@pytest.mark.gpu
@pytest.mark.parametrize("n_passes", VAR_PASSES)
def test_variance_bit_for_bit(_gpu, n_passes):
    for n_floats in VAR_FLOATS:
        for shift in (range(8) if n_floats <= 5 else (0,)):
            m = var_input(n_floats, shift)
            want = R.variance(m, n_passes)
            for om, ov in [(0, 0)] + [(o, 0) for o in (1, 2, 3)] + [(0, o) for o in (1, 2, 3)] + [(o, o) for o in (1, 2, 3)]:
                dm, dv = Buf(m, om), Buf(np.full(n_floats, np.nan, F), ov)
                ptamd.variance(dm.ptr, n_floats, n_passes, dv.ptr)
                assert same(dv.get(), want), (n_floats, shift, om, ov, dv.get(), want)
                dm.get()
    if n_passes == 2 ** 31 - 1:
        assert np.isinf(R.variance(var_input(1), n_passes)[0])


def _gpu_estimate(S, M2, cam, prm, n, off_s=0, off_m=0):
    dS, dM = Buf(S, off_s), Buf(M2, off_m)
    scratch = Buf(np.zeros(ptamd.error_scratch_bytes(S.size) // 4, np.int32))
    e = ptamd.error_estimate(dS.ptr, dM.ptr, cam, prm, n, scratch.ptr)
    scratch.get()
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("case", EST_SMALL + EST_BIG, ids=ids4)
def test_estimate_bit_for_bit(_gpu, case):
    W, H, rank, world = case
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=1, rank=rank, world=world)
    S, M2 = est_slab(W, H, rank, world)
    assert S.size == ptamd.tiles_floats(cam, prm)
    want = R.estimate32(S, M2, EST_N, W, H, rank, world)
    assert want["skipped"] > 0 and want["pixels"] + want["skipped"] == int(R.in_frame(W, H, rank, world).sum())
    for off_s, off_m in ((0, 0), (1, 0), (0, 1)):      # float4 loads; st_estimate<false> either way
        got = _gpu_estimate(S, M2, cam, prm, EST_N, off_s, off_m)
        assert same_estimate(got, want), (case, off_s, off_m, got, want)
    for pad in (np.nan, 1e30):                        # what lies outside the frame is not read into any figure
        Sp, Mp = est_slab(W, H, rank, world, pad=pad)
        got = _gpu_estimate(Sp, Mp, cam, prm, EST_N)
        assert same_estimate(got, want), (case, pad, got, want)


@pytest.mark.gpu
def test_estimate_order_and_degenerate_frames(_gpu):
    W, H, S, M2 = order_frame()
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=1)
    want = R.estimate32(S, M2, 2, W, H)
    for off_s, off_m in ((0, 0), (1, 0), (0, 1)):
        got = _gpu_estimate(S, M2, cam, prm, 2, off_s, off_m)
        assert same_estimate(got, want), (off_s, off_m, got, want)
    W, H = 20, 12
    cam = ptamd.make_camera(W, H)
    z = np.zeros(R.tiles_local(W, H, 1) * 192, F)
    e = _gpu_estimate(z, z, cam, prm, 4)
    assert np.isnan(e["rel_rms"]) and e["mean_rel_se"] == 0.0 and (e["pixels"], e["skipped"]) == (W * H, 0), e
    e = _gpu_estimate(np.full_like(z, np.nan), z, cam, prm, 4)
    assert np.isnan(e["rel_rms"]) and np.isnan(e["mean_rel_se"]) and (e["pixels"], e["skipped"]) == (0, W * H), e


LIST_W, LIST_H = 100, 52                 # 13 x 7 = 91 tiles
BAD_ENTRIES = (-1, 91, 2 ** 31 - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("n_before", (0, 5))
def test_list_fold_skips_entries_outside_the_frame(_gpu, n_before):
    cam = ptamd.make_camera(LIST_W, LIST_H)
    total, passes = 91, 3
    prm = ptamd.default_params(passes=passes)
    lst = np.array([5, -1, 90, 91, 17, 2 ** 31 - 1, 0, 44], np.int32)
    slab = fold_slab(passes, lst.size * 192)
    S0, M0 = fold_state(total * 192, 5)      # a real state also at n_before = 0: what is not listed keeps its bits
    np0 = np.full(total, -7, np.int32)
    dS, dM, dn, dl, work = Buf(S0), Buf(M0), Buf(np0), Buf(lst), Buf(slab)
    ptamd.accumulate_tile_list(work.ptr, cam, prm, dl.ptr, lst.size, n_before, dS.ptr, dM.ptr, dn.ptr)
    gS, gM, gn = dS.get().reshape(total, 192), dM.get().reshape(total, 192), dn.get(np.int32)
    wS, wM, wn = S0.reshape(total, 192).copy(), M0.reshape(total, 192).copy(), np0.copy()
    for e, t in enumerate(lst):
        if 0 <= t < total:
            wS[t], wM[t] = R.fold(slab[:, 192 * e:192 * (e + 1)], wS[t], wM[t], n_before)
            wn[t] = n_before + passes
    listed = np.zeros(total, bool)
    listed[[5, 90, 17, 0, 44]] = True
    assert same(gS[listed], wS[listed]) and same(gM[listed], wM[listed])
    assert np.array_equal(bits(gS[~listed]), bits(wS[~listed])) and np.array_equal(bits(gM[~listed]), bits(wM[~listed]))
    assert np.array_equal(gn, wn)
    work.get(), dl.get(np.int32)


@pytest.mark.gpu
def test_tile_errors_zero_record_outside_the_frame(_gpu):
    W, H, total, n = LIST_W, LIST_H, 91, EST_N
    cam = ptamd.make_camera(W, H)
    S, M2 = est_slab(W, H, 0, 1, pad=np.nan)
    want = A.tile_errors(from_tiles(S, W, H), from_tiles(M2, W, H), n)
    dS, dM = Buf(S), Buf(M2)

    def run(lst, n_tiles):
        derr = Buf(np.full(n_tiles * 4, SENTINEL, np.int32))
        dl = Buf(lst) if lst is not None else None
        ptamd.tile_errors(dS.ptr, dM.ptr, cam, dl.ptr if dl else 0, n_tiles, n, derr.ptr)
        return derr.get(np.int32).view(ptamd.TILE_ERROR_DTYPE)

    lst = np.array([3, -1, 90, 91, 2 ** 31 - 1, 12, 0], np.int32)
    got = run(lst, lst.size)
    for e, t in enumerate(lst):
        g = (got["mean_rel_se"][e:e + 1].view(np.uint64)[0], got["pixels"][e], got["skipped"][e])
        w = (want[0][t:t + 1].view(np.uint64)[0], want[1][t], want[2][t]) if 0 <= t < total else (0, 0, 0)
        assert g == w, (e, t, g, w)
    for n_tiles in (total, 5):               # d_list NULL: entry e is tile e
        got = run(None, n_tiles)
        assert np.array_equal(got["mean_rel_se"].view(np.uint64), want[0][:n_tiles].view(np.uint64))
        assert np.array_equal(got["pixels"], want[1][:n_tiles]) and np.array_equal(got["skipped"], want[2][:n_tiles])
    assert want[2].sum() > 0 and (want[0] > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("outputs", ("mean", "var", "both"))
def test_finish_tiles_bit_for_bit(_gpu, outputs):
    W, H, total = LIST_W, LIST_H, 91
    cam = ptamd.make_camera(W, H)
    counts = np.array([0, 1, 2, 3, 2 ** 24 + 1, 2 ** 31 - 1], np.int32)[np.arange(total) % 6]
    rs = np.random.RandomState(6)
    S = (rs.uniform(0, 1, (H, W, 3)) ** 3 * 40).astype(F)
    M2 = (rs.uniform(0, 1, (H, W, 3)) ** 3 * 9).astype(F)
    for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 2.0 ** 100, 1e-40, -1e-9, 3e38)):      # in every tile, whatever its count
        S[(k % 8)::8, k::8, k % 3] = F(v)
        M2[((k + 3) % 8)::8, k::8, (k + 1) % 3] = F(v)
    wmean, wvar = A.finish(S, M2, counts.reshape(7, 13))
    dS, dM, dn = Buf(A.to_tiles(S)), Buf(A.to_tiles(M2)), Buf(counts)
    nan = np.full(total * 192, np.nan, F)
    dmean, dvar = (Buf(nan) if outputs != "var" else None), (Buf(nan) if outputs != "mean" else None)
    ptamd.finish_tiles(dS.ptr, dM.ptr, dn.ptr, cam, dmean.ptr if dmean else 0, dvar.ptr if dvar else 0)
    inside = A.to_tiles(np.ones((H, W, 1), bool), False)[..., 0]
    for d, w in ((dmean, wmean), (dvar, wvar)):
        if d is not None:
            g = d.get().reshape(total, 64, 3)
            assert same(g[inside], A.to_tiles(w)[inside]), outputs
            assert not bits(g[counts == 0]).any()      # n == 0: +0 in every float of the tile, padding included
    dS.get(), dM.get(), dn.get(np.int32)
