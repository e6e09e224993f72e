"""numpy statement of the denoiser (include/pt_api.h: pt_denoise; csrc/pt_denoise.hip) and of the first-hit feature
buffers it is guided by (pt_render_aov), built from the CPU oracle — test infrastructure only.

Denoiser: edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with albedo demodulation, in float64:
  c_p = rgb_p / sample_cnt;  div_p = albedo_p where > 1e-3 else 1 (per channel; 1 without demodulation);  e_p = c_p / div_p
  finite_p = all three components of e_p are finite (for the input: of c_p)
  iteration i = 0 .. L-1, step s = 2^i, taps q = p + s (dx, dy), dx, dy in -2..2 (dy outer, dx inner), inside the frame and finite_q:
    w = h(dx) h(dy) exp(-E),  h = (1/16, 1/4, 3/8, 1/4, 1/16),
    E = |e_p - e_q|^2 / (sc^2 4^-i)        (left out when !finite_p)
      + |n_p - n_q|^2 / sn^2
      + |z_p - z_q| / (sz max(z_p, z_q))   (0 when both depths are 0)
    w = 0 exactly when E > 80
  e'_p = sum w e_q / sum w, or e_p when sum w = 0;  n (AOV 3..5) and z (AOV 6) stay as they are
  out_p = e_p^(L) div_p sample_cnt;  L = 0 returns the input unchanged.
The edges, as include/pt_api.h states them and both functions below have them: the albedo is compared against the float32 nearest 1e-3
(that value and below divide by 1); E == 80 is used, a NaN E is not; max(z_p, z_q) is the select z_p > z_q ? z_p : z_q and a pair with
max <= 0 (or NaN) adds no depth term; a NaN normal, or a depth of +inf, makes every E of the pixel NaN: it keeps its value and is
nobody's tap.

`denoise` is the definition in float64.  `denoise32` is the three kernels of csrc/pt_denoise.hip restated in float32, every operation
rounded once and in the kernels' order — the one operation it cannot replay is the device's expf, which is a parameter.  On inputs
whose every exp argument is 0 the weights are the dyadic h products and the GPU returns denoise32's bits (tests/test_denoise_exact.py).
"""
import numpy as np

H_TAPS = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float64)
THRESHOLD = np.float32(1e-3)      # the kernel's 1e-3f: 0x3A83126F = 0.001000000047...
F32 = np.float32
DEFAULTS = dict(iterations=5, sigma_color=16.0, sigma_normal=0.1, sigma_depth=0.1, demodulate=1)      # pt_denoise_params_default


def denoise(rgb, aov, sample_cnt, iterations=5, sigma_color=16.0, sigma_normal=0.1, sigma_depth=0.1, demodulate=1):
    """rgb (H, W, 3), aov (H, W, 8) -> (H, W, 3) float64, as defined above."""
    rgb = np.asarray(rgb, np.float64)
    aov = np.asarray(aov, np.float64)
    if iterations == 0:
        return rgb.copy()
    Hh, Ww = rgb.shape[:2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = rgb / float(sample_cnt)
        div = np.where(aov[..., 0:3] > THRESHOLD, aov[..., 0:3], 1.0) if demodulate else np.ones_like(c)
        e = c / div
    fin = np.isfinite(c).all(-1)
    n, z = aov[..., 3:6], aov[..., 6]
    kn, kz = 1.0 / (sigma_normal * sigma_normal), 1.0 / sigma_depth
    for i in range(iterations):
        s = 1 << i
        kc = (4.0 ** i) / (sigma_color * sigma_color)
        acc = np.zeros_like(e)
        wsum = np.zeros((Hh, Ww))
        ys, xs = np.arange(Hh), np.arange(Ww)
        for dy in range(-2, 3):
            qy = ys + s * dy
            vy = (qy >= 0) & (qy < Hh)
            qyc = np.clip(qy, 0, Hh - 1)
            for dx in range(-2, 3):
                qx = xs + s * dx
                vx = (qx >= 0) & (qx < Ww)
                qxc = np.clip(qx, 0, Ww - 1)
                eq, nq, zq, fq = (a[qyc][:, qxc] for a in (e, n, z, fin))
                ok = vy[:, None] & vx[None, :] & fq
                with np.errstate(invalid="ignore", over="ignore"):
                    dc = ((e - eq) ** 2).sum(-1) * kc
                    E = np.where(fin, dc, 0.0) + ((n - nq) ** 2).sum(-1) * kn
                    mz = np.where(z > zq, z, zq)
                    E = E + np.where(mz > 0, np.abs(z - zq) * kz / np.where(mz > 0, mz, 1.0), 0.0)
                    w = np.where(ok & (E <= 80.0), H_TAPS[dx + 2] * H_TAPS[dy + 2] * np.exp(-np.where(ok, E, 0.0)), 0.0)
                    acc += w[..., None] * np.where(ok[..., None], eq, 0.0)
                wsum += w
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.where((wsum > 0)[..., None], acc / np.where(wsum > 0, wsum, 1.0)[..., None], e)
        fin = np.isfinite(e).all(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        return e * div * float(sample_cnt)


def exp32(x):
    """exp of float32 arguments, correctly rounded to float32 (through float64)."""
    return np.exp(np.asarray(x, np.float64)).astype(F32)


def denoise32(rgb, aov, sample_cnt, iterations=5, sigma_color=16.0, sigma_normal=0.1, sigma_depth=0.1, demodulate=1, exp_fn=exp32):
    """rgb (H, W, 3), aov (H, W, 8) -> (H, W, 3) float32: dn_pack, L x dn_atrous, dn_finish in float32, one rounding per operation.
    exp_fn gets the float32 array -E of the taps that are used (one call per tap offset) and returns their float32 exponentials."""
    rgb = np.ascontiguousarray(rgb, F32)
    aov = np.ascontiguousarray(aov, F32)
    if iterations == 0:
        return rgb.copy()
    Hh, Ww = rgb.shape[:2]
    one, cnt = F32(1), F32(int(sample_cnt))                      # (float)sample_cnt: round to nearest even
    sc, sn, sz = F32(sigma_color), F32(sigma_normal), F32(sigma_depth)
    h = H_TAPS.astype(F32)
    with np.errstate(all="ignore"):
        # dn_pack
        c = rgb / cnt
        alb = aov[..., 0:3]
        div = np.where(alb > THRESHOLD, alb, one) if demodulate else np.ones_like(c)
        e = c / div
        fin = np.isfinite(c).all(-1)
        n, z = aov[..., 3:6], aov[..., 6]
        kn, kz, kc = one / (sn * sn), one / sz, one / (sc * sc)
        ys, xs = np.arange(Hh), np.arange(Ww)
        for i in range(iterations):                              # dn_atrous at step 2^i
            s = 1 << i
            acc = np.zeros_like(e)
            wsum = np.zeros((Hh, Ww), F32)
            for dy in range(-2, 3):
                qy = ys + s * dy
                vy = (qy >= 0) & (qy < Hh)
                qyc = np.clip(qy, 0, Hh - 1)
                for dx in range(-2, 3):
                    qx = xs + s * dx
                    vx = (qx >= 0) & (qx < Ww)
                    qxc = np.clip(qx, 0, Ww - 1)
                    eq, nq, zq, fq = (a[qyc][:, qxc] for a in (e, n, z, fin))
                    d = e - eq
                    E = np.where(fin, ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * kc, F32(0))
                    d = n - nq
                    E = E + ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * kn
                    mz = np.where(z > zq, z, zq)
                    E = np.where(mz > 0, E + (np.abs(z - zq) * kz) / mz, E)
                    use = vy[:, None] & vx[None, :] & fq & (E <= F32(80))
                    w = np.zeros((Hh, Ww), F32)
                    w[use] = (h[dx + 2] * h[dy + 2]) * np.asarray(exp_fn(-E[use]), F32)
                    acc = np.where(use[..., None], acc + w[..., None] * eq, acc)
                    wsum = np.where(use, wsum + w, wsum)
            o = acc / wsum[..., None]
            got = wsum > 0
            e = np.where(got[..., None], o, e)
            fin = np.where(got, np.isfinite(o).all(-1), fin)
            kc = kc * F32(4)
        return (e * div) * cnt                                   # dn_finish


def aov_from_oracle(oscene, ocam, W, H, passes, first_pass):
    """The first-hit feature buffers (pt_render_aov) accumulated on the host from the oracle, in float32 and pass order:
    (H, W, 8) float32 and the primitive of pass first_pass (H, W) int32.  oscene: oracle_lib.Scene, ocam: oracle_lib.make_camera."""
    import oracle_lib as O
    py, px = np.mgrid[0:H, 0:W]
    acc = np.zeros((H * W, 8), np.float32)
    hits = np.zeros(H * W, np.float32)
    prim0 = None
    pos = np.array(ocam.pos[:], np.float32)
    for j in range(passes):
        rows = np.stack([px.ravel(), py.ravel(), np.full(H * W, first_pass + j)], 1).astype(np.int32)
        d = O.pixel_dir(ocam, rows)[:, 2:5]
        rays = np.concatenate([np.broadcast_to(pos, (H * W, 3)), d, np.zeros((H * W, 1), np.float32),
                               np.full((H * W, 1), 999999.0, np.float32)], 1).astype(np.float32)
        h, prim, _ = oscene.raycast(rays)
        hit = prim >= 0
        acc[hit, 0:3] = acc[hit, 0:3] + h[hit, 20:23]
        acc[hit, 3:6] = acc[hit, 3:6] + h[hit, 8:11]
        acc[hit, 6] = acc[hit, 6] + h[hit, 1]
        hits[hit] = hits[hit] + np.float32(1)
        if j == 0:
            prim0 = prim.astype(np.int32)
    out = np.zeros((H * W, 8), np.float32)
    out[:, 0:6] = acc[:, 0:6] / np.float32(passes)
    nz = hits > 0
    out[nz, 6] = acc[nz, 6] / hits[nz]
    out[:, 7] = hits / np.float32(passes)
    return out.reshape(H, W, 8), prim0.reshape(H, W)


def rel_rms_finite(a, ref):
    """Relative RMS of a against ref over the pixels where both are finite."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    m = np.isfinite(a).all(-1) & np.isfinite(ref).all(-1)
    return float(np.sqrt(((a[m] - ref[m]) ** 2).sum() / (ref[m] ** 2).sum()))
