"""numpy statement of the moments over passes and of the error estimate reduced from them (include/pt_api.h:
pt_accumulate_passes, pt_variance, pt_error_estimate; csrc/pt_stats.hip) — test infrastructure only.

Fold, per float, pass k = n_before + 1, ... with mean m, every operation IEEE float32 in this order:
  S_prev = S;  S = S_prev + m                                                  (k = 1: S = 0 + m)
  k >= 2:  d1 = m - S_prev / (k - 1);  d2 = m - S / k;  M2 = M2 + d1 * d2      (k = 1: M2 = 0)
Var = max(M2, 0) * n / (n - 1) (a NaN M2 stays NaN): the estimated variance of S.
Estimate over the pixels whose S and M2 are all finite, per-pixel terms in float32 as written, sums in float64:
  rel_rms     = sqrt( sum Var_c / sum S_c * S_c )
  mean_rel_se = mean of sqrt((Var_r + Var_g) + Var_b) / (((|S_r| + |S_g|) + |S_b|) + 0.03 n)
"""
import numpy as np

F = np.float32


def fold(means, S=None, M2=None, n_before=0):
    """means: (passes, ...) float32 per-pass means.  Returns (S, M2) float32 after folding them into the given state
    (n_before = 0: the state is not read)."""
    means = np.asarray(means, F)
    if n_before == 0:
        S, M2 = np.zeros(means.shape[1:], F), np.zeros(means.shape[1:], F)
    else:
        S, M2 = np.array(S, F), np.array(M2, F)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(means.shape[0]):
            k = n_before + j + 1
            m = means[j]
            Sp = S
            S = Sp + m
            if k >= 2:
                d1 = m - Sp / F(k - 1)
                d2 = m - S / F(k)
                M2 = M2 + d1 * d2
    assert S.dtype == F and M2.dtype == F
    return S, M2


def sumsq_form(means):
    """The BANNED form of M2, Q - S^2 / n in float32 — here only to show why it is banned."""
    means = np.asarray(means, F)
    S, Q = np.zeros(means.shape[1:], F), np.zeros(means.shape[1:], F)
    for m in means:
        S = S + m
        Q = Q + m * m
    return Q - S * S / F(means.shape[0])


def variance(M2, n):
    M2 = np.asarray(M2, F)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.where(M2 < 0, F(0), M2) * F(n)) / F(n - 1)


def estimate(S, M2, n):
    """S, M2: (..., 3) float32.  Returns dict(rel_rms, mean_rel_se, pixels, skipped)."""
    S, M2 = np.asarray(S, F).reshape(-1, 3), np.asarray(M2, F).reshape(-1, 3)
    ok = np.isfinite(S).all(-1) & np.isfinite(M2).all(-1)
    s, v = S[ok], variance(M2[ok], n)
    assert v.dtype == F
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        se = np.sqrt((v[:, 0] + v[:, 1]) + v[:, 2]) / (((np.abs(s[:, 0]) + np.abs(s[:, 1])) + np.abs(s[:, 2])) + F(0.03) * F(n))
        assert se.dtype == F
        rel_rms = float(np.sqrt(v.astype(np.float64).sum() / (s * s).astype(np.float64).sum()))
        mean_rel_se = float(se.astype(np.float64).sum() / ok.sum())
    return dict(rel_rms=rel_rms, mean_rel_se=mean_rel_se, pixels=int(ok.sum()), skipped=int((~ok).sum()))


TILE, EST_BLOCKS, EST_THREADS = 8, 1024, 256
# estimate32(wrong=...): one deliberate departure from st_estimate each, for the sensitivity tests of tests/test_stats_exact.py
EST_WRONG = ("one_trip", "rank_ignored", "padding_counted", "channels_in_float32", "finite_s_only", "bias_in_float64", "waves_reversed",
             "blocks_reversed")


def tiles_local(W, H, world):
    tx, ty = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    return (tx * ty + world - 1) // world


def in_frame(W, H, rank, world, n_tiles_local=None):
    """(n_tiles_local * 64,) bool: the pixels of rank's tile-layout slab whose tile exists and that lie inside W x H.  Slab tile i is
    frame tile i * world + rank (row-major over the tile grid), pixel = ty * 8 + tx inside it."""
    tx, ty = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    q = np.arange((tiles_local(W, H, world) if n_tiles_local is None else n_tiles_local) * 64, dtype=np.int64)
    tile, lane = (q >> 6) * world + rank, q & 63
    return (tile < tx * ty) & ((tile % tx) * TILE + (lane & 7) < W) & ((tile // tx) * TILE + (lane >> 3) < H)


def _tree64(a):
    """adaptive_ref.tree_sum: (..., 64) float64 -> (...) in the order of the wave reduction (lane l < o adds lane l + o, o = 32 .. 1)."""
    from adaptive_ref import tree_sum
    return tree_sum(a)


def estimate32(S, M2, n, W, H, rank=0, world=1, wrong=None):
    """pt_error_estimate as the kernel st_estimate and its host sum compute it, in their order: same bits.
    S, M2: rank's tile-layout slab, n_tiles_local * 192 float32 each.  nb = min(1024, ceil(floats / 3072)) blocks of 256 threads; thread t
    of the grid takes the groups t, t + nb * 256, ... of 4 pixels; a pixel whose tile does not exist or that lies outside W x H is passed
    over, one with a non-finite S or M2 is counted as skipped; per pixel used, float32 v = (max(M2, 0) nf) / nf1 and bias = 0.03f nf,
      aVar += v_r; += v_g; += v_b;   aS2 += f64(s_r s_r); ... g, b;   aSe += f64(sqrtf((v_r + v_g) + v_b) / (((|s_r| + |s_g|) + |s_b|) + bias))
    into float64 accumulators that start at 0.0; per wave the shuffle tree, per block ((w0 + w1) + w2) + w3, on the host 0.0 + p0 + p1 +
    ...; rel_rms = sqrt(var / s2), mean_rel_se = se / pixels.  Returns dict(rel_rms, mean_rel_se, pixels, skipped)."""
    assert wrong is None or wrong in EST_WRONG
    S, M2 = np.asarray(S, F).reshape(-1), np.asarray(M2, F).reshape(-1)
    n_floats = S.size
    assert n_floats == M2.size and n_floats % 192 == 0 and n_floats > 0
    nb = min(EST_BLOCKS, (n_floats + 3071) // 3072)
    T = nb * EST_THREADS
    n_groups = n_floats // 12
    trips = (n_groups + T - 1) // T
    here = in_frame(W, H, 0 if wrong == "rank_ignored" else rank, world, n_floats // 192)
    if wrong == "padding_counted":
        here = np.ones_like(here)
    pad = trips * T * 4 - here.size                       # groups past the last: no thread reads them
    here = np.concatenate([here, np.zeros(pad, bool)]).reshape(trips, T, 4)
    s = np.concatenate([S, np.zeros(pad * 3, F)]).reshape(trips, T, 4, 3)
    m = np.concatenate([M2, np.zeros(pad * 3, F)]).reshape(trips, T, 4, 3)
    fin = np.isfinite(s).all(-1) & (True if wrong == "finite_s_only" else np.isfinite(m).all(-1))
    used = here & fin
    nf, nf1 = F(n), F(n - 1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        v = variance(m, n)
        s2 = s * s
        root = np.sqrt((v[..., 0] + v[..., 1]) + v[..., 2])
        mag = (np.abs(s[..., 0]) + np.abs(s[..., 1])) + np.abs(s[..., 2])
        if wrong == "bias_in_float64":
            se = root.astype(np.float64) / (mag.astype(np.float64) + 0.03 * np.float64(nf))
        else:
            se = (root / (mag + F(0.03) * nf)).astype(np.float64)
        assert v.dtype == F and s2.dtype == F and root.dtype == F and nf1.dtype == F
        aVar, aS2, aSe = np.zeros(T), np.zeros(T), np.zeros(T)
        for trip in range(1 if wrong == "one_trip" else trips):
            for j in range(4):
                u = used[trip, :, j]
                if wrong == "channels_in_float32":
                    aVar = np.where(u, aVar + ((v[trip, :, j, 0] + v[trip, :, j, 1]) + v[trip, :, j, 2]).astype(np.float64), aVar)
                    aS2 = np.where(u, aS2 + ((s2[trip, :, j, 0] + s2[trip, :, j, 1]) + s2[trip, :, j, 2]).astype(np.float64), aS2)
                else:
                    for c in range(3):
                        aVar = np.where(u, aVar + v[trip, :, j, c].astype(np.float64), aVar)
                        aS2 = np.where(u, aS2 + s2[trip, :, j, c].astype(np.float64), aS2)
                aSe = np.where(u, aSe + se[trip, :, j], aSe)
        tot = []
        for a in (aVar, aS2, aSe):
            w = _tree64(a.reshape(nb, 4, 64))            # (nb, 4): lane 0 of every wave
            if wrong == "waves_reversed":
                w = w[:, ::-1]
            p = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
            t = np.float64(0.0)
            for b in (range(nb - 1, -1, -1) if wrong == "blocks_reversed" else range(nb)):
                t = t + p[b]
            tot.append(t)
        seen = slice(0, 1) if wrong == "one_trip" else slice(None)
        pixels, skipped = int(used[seen].sum()), int((here & ~fin)[seen].sum())
        rel_rms = float(np.sqrt(tot[0] / tot[1]))
        mean_rel_se = float(tot[2] / np.float64(pixels))
    return dict(rel_rms=rel_rms, mean_rel_se=mean_rel_se, pixels=pixels, skipped=skipped)


def summation_bound(n_floats, pixels):
    """Relative bound between estimate32's sums and R.estimate's, both of non-negative float64 terms: a sum of terms each added with one
    rounding is within (additions on the longest path) * 2^-53 of the exact sum, to first order.  estimate32: 12 additions per trip (4
    pixels x 3 channels) in a thread, 6 levels of the wave tree, 3 for the waves, nb for the blocks; numpy's pairwise sum of N terms:
    log2 N.  The quotient of two such sums doubles it and the square root halves it again; mean_rel_se has 4 additions per trip."""
    nb = min(1024, (n_floats + 3071) // 3072)
    trips = -(-(n_floats // 12) // (nb * 256))
    return (12 * trips + 6 + 3 + nb + np.log2(3 * pixels)) * 2.0 ** -53
