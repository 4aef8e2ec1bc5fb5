"""A float64 numpy model of one level of the denoiser's filter (include/rtx.h rtx_denoise_params,
DESIGN §7.5) and the synthetic frame test_gpu_denoise.py filters.  The model shifts whole arrays per
tap, so a level of a small frame takes milliseconds."""
import numpy as np

from rtxpy import abi

H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float64)
SIGMAS = {"sigma_color": 0.6, "sigma_normal": 0.3, "sigma_albedo": 0.1, "sigma_plane": 0.02}
TERMS = ("color", "normal", "albedo", "plane")


def live_mask(c, feat):
    """pixels that take part in a level: a hit (z != 0) with a finite colour"""
    return (feat["z"] != 0) & np.isfinite(c).all(axis=-1)


def level(c, feat, k, sigmas=SIGMAS, without=None):
    """level k (step 2^k, sigma_color * 2^-k) of the filter over colour c (h, w, 3) and features feat
    (h, w) of abi.FEATURE_DTYPE, in float64; `without` names a term of e to leave out.  Pixels that are
    not live come back as they are."""
    h, w = c.shape[:2]
    s = 1 << k
    live = live_mask(c, feat)
    c64 = np.where(live[..., None], c, 0).astype(np.float64)
    z, P, n, a = (feat[f].astype(np.float64) for f in ("z", "position", "normal", "albedo"))
    inv = {t: 0.0 if t == without else 1.0 / float(sigmas["sigma_" + t]) ** 2 for t in TERMS}
    inv["color"] *= 4.0 ** k
    num, den = np.zeros((h, w, 3)), np.zeros((h, w))
    for v in range(-2, 3):
        for u in range(-2, 3):
            dy, dx = v * s, u * s
            y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            D = (slice(y0, y1), slice(x0, x1))
            S = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            ok = live[D] & live[S]
            zi = np.where(z[D] != 0, z[D], 1.0)
            e = (((c64[D] - c64[S]) ** 2).sum(-1) * inv["color"] + ((n[D] - n[S]) ** 2).sum(-1) * inv["normal"]
                 + ((a[D] - a[S]) ** 2).sum(-1) * inv["albedo"]
                 + (n[D] * (P[S] - P[D])).sum(-1) ** 2 * inv["plane"] / zi ** 2)
            wgt = np.where(ok, H5[u + 2] * H5[v + 2] * np.exp(-e), 0.0)
            num[D] += wgt[..., None] * c64[S]
            den[D] += wgt
    out = np.array(c, np.float64)
    out[live] = num[live] / den[live][:, None]
    return out


def synthetic(W=37, H=29):
    """(rgb (H, W, 3) float32, features (H, W)): two surfaces that meet at the middle column (a flat one
    with a depth ramp, a curved one), a band of misses, a checkerboard albedo, noise, one NaN, one inf"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(x - W / 2) / W, (y - H / 2) / W, np.ones_like(x)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    left = x < W // 2
    z = np.where(left, 4 + 2 * y / H, 7 - 1.5 * x / W)
    a_, b_ = (x - 0.75 * W) / (0.3 * W), (y - H / 2) / (0.6 * H)
    nr = np.stack([a_, b_, -np.sqrt(np.maximum(1 - a_ * a_ - b_ * b_, 0.05))], -1)
    nr /= np.linalg.norm(nr, axis=-1, keepdims=True)
    n = np.where(left[..., None], np.array([0.0, 0.0, -1.0]), nr)
    miss = (np.abs(x - W // 2) <= 1) & (y < 10)
    check = ((x // 4 + y // 4) % 2).astype(bool)
    alb = np.where(check[..., None], np.array([0.15, 0.2, 0.6]), np.array([0.9, 0.85, 0.8]))
    rgb = alb * (0.6 + 0.3 * np.sin(x / 5))[..., None] + np.abs(np.random.default_rng(5).normal(0, 0.25, (H, W, 3)))
    rgb[miss] = 0.05
    rgb = rgb.astype(np.float32)
    rgb[5, 7, 1] = np.nan
    rgb[20, 30, 0] = np.inf
    feat = np.zeros((H, W), abi.FEATURE_DTYPE)
    feat["z"] = z
    feat["position"] = d * z[..., None]
    feat["normal"] = n
    feat["albedo"] = alb
    feat["material"] = check
    feat["object"] = np.where(left, 0, 1)
    hit = ~miss
    for f in ("z", "position", "normal", "albedo"):
        feat[f] = np.where(hit.reshape(hit.shape + (1,) * (feat[f].ndim - 2)), feat[f], 0)
    feat["material"][miss] = -1
    feat["object"][miss] = -1
    return rgb, feat


def finite_max(c):
    return float(np.abs(c[np.isfinite(c)]).max())
