"""numpy statement of the per-tile error figure and of the adaptive stopping loop (include/pt_api.h: pt_tile_errors, pt_finish_tiles,
pt_render_adaptive; csrc/pt_stats.hip) — test infrastructure only.  Builds on stats_ref.py (the fold and the variance).

Tile error, for the 8x8 tile t of a W x H frame with moments S, M2 of n passes: a pixel is used if it lies inside the frame and its six
floats are finite; per used pixel, float32 as written,
  v_c = max(M2_c, 0) * n / (n - 1);   term = sqrt((v_r + v_g) + v_b) / (((|S_r| + |S_g|) + |S_b|) + 0.03f * n)
(0.0 for a pixel not used); the 64 terms, as float64, are summed in the tree  for o = 32, 16, 8, 4, 2, 1: pixel l < o adds pixel l + o
(pixel = ty * 8 + tx); err = sum / pixels in float64, 0 when there is none.
Loop: the active list starts as all tiles; each round adds b = min(batch, max_passes - done) passes to every active tile; once
done >= max(min_passes, 2) the errors of the active tiles are taken and every tile with err <= target leaves the list (a NaN stays).
"""
import numpy as np

import stats_ref as R

F = np.float32
TILE = 8


def tile_grid(W, H):
    return (H + TILE - 1) // TILE, (W + TILE - 1) // TILE      # tiles_y, tiles_x


def to_tiles(frame, fill=0):
    """(H, W, C) -> (tiles, 64, C), tiles row-major, pixel = ty * 8 + tx; pixels outside the frame hold `fill`."""
    H, W, ch = frame.shape
    ty, tx = tile_grid(W, H)
    pad = np.full((ty * TILE, tx * TILE, ch), fill, frame.dtype)
    pad[:H, :W] = frame
    return pad.reshape(ty, TILE, tx, TILE, ch).transpose(0, 2, 1, 3, 4).reshape(ty * tx, TILE * TILE, ch)


def tree_sum(terms):
    """(..., 64) -> (...) float64 in the order of the wave reduction."""
    a = np.array(terms, np.float64)
    assert a.shape[-1] == 64
    for o in (32, 16, 8, 4, 2, 1):
        a[..., :o] = a[..., :o] + a[..., o:2 * o]
    return a[..., 0].copy()


def tile_errors(S, M2, n):
    """S, M2: (H, W, 3) float32 moments of n passes.  Returns (err float64, pixels int32, skipped int32), one entry per tile, row-major."""
    S, M2 = np.asarray(S, F), np.asarray(M2, F)
    H, W = S.shape[:2]
    inside = to_tiles(np.ones((H, W, 1), bool), False)[..., 0]
    s, m = to_tiles(S), to_tiles(M2)
    used = inside & np.isfinite(s).all(-1) & np.isfinite(m).all(-1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        v = R.variance(m, n)
        term = np.sqrt((v[..., 0] + v[..., 1]) + v[..., 2]) / (((np.abs(s[..., 0]) + np.abs(s[..., 1])) + np.abs(s[..., 2])) + F(0.03) * F(n))
    assert term.dtype == F
    total = tree_sum(np.where(used, term, F(0)).astype(np.float64))
    pixels = used.sum(-1).astype(np.int32)
    skipped = (inside & ~used).sum(-1).astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(pixels > 0, total / pixels.astype(np.float64), 0.0)
    return err, pixels, skipped


def finish(S, M2, tile_passes):
    """mean = S / n and Var = max(M2, 0) * n / (n - 1) with n the tile's own pass count (n == 0: +0); (H, W, 3) float32 each."""
    S, M2 = np.asarray(S, F), np.asarray(M2, F)
    H, W = S.shape[:2]
    n = np.repeat(np.repeat(np.asarray(tile_passes, np.int32), TILE, 0), TILE, 1)[:H, :W, None]
    nf, nf1 = n.astype(F), (n - 1).astype(F)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        mean = np.where(n == 0, F(0), S / nf)
        var = np.where(n == 0, F(0), (np.where(M2 < 0, F(0), M2) * nf) / nf1)
    assert mean.dtype == F and var.dtype == F
    return mean, var


def adaptive_loop(means, target, batch, min_passes, max_passes):
    """means: (P, H, W, 3) float32 stack of per-pass frames, P >= max_passes.  Returns dict(tile_passes (ty, tx) int32, tile_err (ty, tx)
    float64 at the tile's last check, S, M2 (H, W, 3) with every tile at its own pass count, rounds, converged, max_err, work (tile-passes),
    checks: the list of (passes in, errors of the tiles active at that check))."""
    means = np.asarray(means, F)
    H, W = means.shape[1:3]
    ty, tx = tile_grid(W, H)
    batch = min(batch, max_passes)
    min_passes = max(min_passes, 2)
    assert batch >= 1 and min_passes <= max_passes <= means.shape[0] and target >= 0
    active = np.ones(ty * tx, bool)
    passes = np.zeros(ty * tx, np.int32)
    last = np.zeros(ty * tx, np.float64)
    S = M2 = None
    outS, outM = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F)
    done = rounds = work = 0
    checks = []

    def pixel_mask(tiles):
        return np.repeat(np.repeat(tiles.reshape(ty, tx), TILE, 0), TILE, 1)[:H, :W]

    while active.any() and done < max_passes:
        b = min(batch, max_passes - done)
        S, M2 = R.fold(means[done:done + b], S, M2, done)      # the whole frame; only the active tiles are looked at
        done += b
        rounds += 1
        work += int(active.sum()) * b
        passes[active] = done
        m = pixel_mask(active)
        outS[m], outM[m] = S[m], M2[m]
        if done < min_passes:
            continue
        err, _, _ = tile_errors(S, M2, done)
        last[active] = err[active]
        checks.append((done, err[active].copy()))
        active &= ~(err <= target)
    return dict(tile_passes=passes.reshape(ty, tx), tile_err=last.reshape(ty, tx), S=outS, M2=outM, rounds=rounds,
                converged=int((last <= target).sum()), max_err=float(last[~np.isnan(last)].max()), work=work, checks=checks)
