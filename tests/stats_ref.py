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
