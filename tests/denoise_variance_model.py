"""A float64 numpy model of one level of the variance-guided filter (include/rtx.h
rtx_denoise_variance_params) and the variance that goes with denoise_model.synthetic().
Like denoise_model.py it shifts whole arrays per tap."""
import numpy as np

import denoise_model as DM
from denoise_model import H5, TERMS, finite_max, synthetic  # noqa: F401

B3 = np.array([1 / 4, 1 / 2, 1 / 4], np.float64)
SIGMAS = {"sigma_color": 2.0, "sigma_normal": 0.3, "sigma_albedo": 0.1, "sigma_plane": 0.02}


def live_mask(c, V, feat):
    """pixels that take part in a level: denoise_model's (a hit with a finite colour) with every variance
    component finite and >= 0"""
    with np.errstate(invalid="ignore"):
        return DM.live_mask(c, feat) & np.isfinite(V).all(axis=-1) & (V >= 0).all(axis=-1)


def shifted(h, w, dy, dx):
    """(destination, source) slices of the pixels whose tap at (dy, dx) lies inside the frame, or None"""
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def local_noise(V, live):
    """g: the 3 x 3 mean of V_r + V_g + V_b over the adjacent live pixels, weights B3 x B3 normalised by those
    used (0 where no adjacent pixel is live)"""
    h, w = live.shape
    s = np.where(live, np.where(live[..., None], V, 0).sum(-1), 0.0)
    num, den = np.zeros((h, w)), np.zeros((h, w))
    for v in range(-1, 2):
        for u in range(-1, 2):
            sl = shifted(h, w, v, u)
            if sl is None:
                continue
            D, S = sl
            num[D] += B3[u + 1] * B3[v + 1] * s[S]
            den[D] += B3[u + 1] * B3[v + 1] * live[S]
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def level(c, V, feat, k, sigmas=SIGMAS, without=None):
    """level k (step 2^k; sigma_color is the same at every level) over colour c and variance V (h, w, 3) and
    features feat (h, w) of abi.FEATURE_DTYPE, in float64; `without` names a term of e to leave out.  Returns
    (colour, variance); pixels that are not live come back as they are."""
    h, w = c.shape[:2]
    s = 1 << k
    live = live_mask(c, V, feat)
    c64 = np.where(live[..., None], c, 0).astype(np.float64)
    V64 = np.where(live[..., None], V, 0).astype(np.float64)
    z, P, n, a = (feat[f].astype(np.float64) for f in ("z", "position", "normal", "albedo"))
    inv = {t: 0.0 if t == without else 1.0 / float(sigmas["sigma_" + t]) ** 2 for t in TERMS}
    g = local_noise(V64, live)
    num, var, den = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w))
    for v in range(-2, 3):
        for u in range(-2, 3):
            sl = shifted(h, w, v * s, u * s)
            if sl is None:
                continue
            D, S = sl
            ok = live[D] & live[S]
            zi = np.where(z[D] != 0, z[D], 1.0)
            d2 = ((c64[D] - c64[S]) ** 2).sum(-1)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                ec = np.where((d2 == 0) | (inv["color"] == 0), 0.0, d2 * inv["color"] / (2.0 * g[D]))
                e = (ec + ((n[D] - n[S]) ** 2).sum(-1) * inv["normal"] + ((a[D] - a[S]) ** 2).sum(-1) * inv["albedo"]
                     + (n[D] * (P[S] - P[D])).sum(-1) ** 2 * inv["plane"] / zi ** 2)
                wgt = H5[u + 2] * H5[v + 2] * np.exp(-e)
            wgt = np.where(ok & (wgt >= 0), wgt, 0.0)  # a NaN e weighs nothing
            num[D] += wgt[..., None] * (c64[S] - c64[D])
            var[D] += (wgt * wgt)[..., None] * V64[S]
            den[D] += wgt
    out_c, out_v = np.array(c, np.float64), np.array(V, np.float64)
    out_c[live] = c64[live] + num[live] / den[live][:, None]
    out_v[live] = var[live] / (den[live] ** 2)[:, None]
    return out_c, out_v


def synthetic_variance(rgb, K=4):
    """the variance of the mean that goes with synthetic()'s rgb (whose noise has sd 0.25): (0.25 r)^2 / K with r
    uniform in [0.5, 1.5) per pixel and channel, a block and two single pixels of zero variance, one NaN, one
    negative and one infinite component.  With it every term of e decides something at levels 0 and 1."""
    h, w = rgb.shape[:2]
    r = np.random.default_rng(9).uniform(0.5, 1.5, (h, w, 3))
    V = ((0.25 * r) ** 2 / K).astype(np.float32)
    V[12:15, 3:6] = 0.0      # its centre's g is 0: only taps of exactly its colour weigh
    V[2, 30] = 0.0
    V[25, 12] = 0.0
    V[8, 25, 2] = np.nan     # live for rtx_denoise, not here
    V[17, 9, 0] = -1e-3
    V[22, 33, 1] = np.inf
    return V
