"""A float64 numpy model of the feature-guided upsampler and of the refinement list (include/rtx.h rtx_upsample*,
rtx_upsample_tiles*), and the synthetic pair of frames test_gpu_upsample.py upsamples.  The model gathers
whole arrays per tap, so a small frame takes milliseconds."""
import numpy as np

from rtxpy import abi

SIGMAS = {"sigma_normal": 0.3, "sigma_albedo": 0.1, "sigma_plane": 0.02}
TERMS = ("normal", "albedo", "plane", "material")
F32 = lambda x: float(np.float32(x))  # noqa: E731


def low_size(n, s):
    return -(-n // s)


def axis_taps(n, s):
    """per full coordinate X = 0..n-1: x0 = floor(u) and fx = u - x0 of u = (X - (s - 1) / 2) / s, from integers as
    the header writes them"""
    num = 2 * np.arange(n, dtype=np.int64) - (s - 1)
    x0 = num // (2 * s)
    return x0, (num - 2 * s * x0) / (2.0 * s)


def upsample(low_rgb, low_feat, feat, s, sigmas=SIGMAS, match_material=True, demodulate=False, albedo_min=1.0 / 64.0,
             without=None):
    """the header's formulas in float64.  Returns a dict: rgb (h, w, 3), conf (h, w), bilinear (h, w, 3) (the plain
    bilinear mean over the considered taps of finite colour, 0 where there is none: the fallback everywhere), R (the
    largest demodulation factor used), margin (the least |e - E_MAX| over the hit taps, relative to E_MAX).
    `without` names a term to leave out: normal, albedo, plane, or material (the material match)."""
    h, w = feat.shape
    lh, lw = low_feat.shape
    assert (lh, lw) == (low_size(h, s), low_size(w, s)) and low_rgb.shape == (lh, lw, 3)
    x0, fx = axis_taps(w, s)
    y0, fy = axis_taps(h, s)
    inv = {t: 0.0 if t == without else 1.0 / F32(sigmas["sigma_" + t]) ** 2 for t in ("normal", "albedo", "plane")}
    zp, Pp, n_p, ap = (feat[f].astype(np.float64) for f in ("z", "position", "normal", "albedo"))
    hit_p = feat["z"] != 0
    zi = np.where(hit_p, zp, 1.0)
    amin = F32(albedo_min)
    num, den, ball = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
    bnum, bden = np.zeros((h, w, 3)), np.zeros((h, w))
    R, margin = 1.0, np.inf
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0 + i, y0 + j
            b = (fy if j else 1 - fy)[:, None] * (fx if i else 1 - fx)[None, :]
            inside = ((qy >= 0) & (qy < lh))[:, None] & ((qx >= 0) & (qx < lw))[None, :] & (b > 0)
            Q = (np.clip(qy, 0, lh - 1)[:, None], np.clip(qx, 0, lw - 1)[None, :])
            c = low_rgb[Q].astype(np.float64)
            fq = low_feat[Q]
            fin = inside & np.isfinite(c).all(-1)
            c = np.where(fin[..., None], c, 0.0)
            ball += np.where(inside, b, 0.0)
            bnum += np.where(fin, b, 0.0)[..., None] * c
            bden += np.where(fin, b, 0.0)
            hit_q = fq["z"] != 0
            nq, aq, Pq = (fq[f].astype(np.float64) for f in ("normal", "albedo", "position"))
            with np.errstate(invalid="ignore", over="ignore"):
                e = (((n_p - nq) ** 2).sum(-1) * inv["normal"] + ((ap - aq) ** 2).sum(-1) * inv["albedo"]
                     + (n_p * (Pq - Pp)).sum(-1) ** 2 * inv["plane"] / zi ** 2)
            same = np.ones((h, w), bool) if (not match_material or without == "material") else feat["material"] == fq["material"]
            cand = fin & hit_p & hit_q & same
            if cand.any():
                margin = min(margin, float(np.nanmin(np.abs(e[cand] / abi.RTX_UPSAMPLE_E_MAX - 1))))
            g = np.where(~hit_p & ~hit_q, 1.0, np.where(cand & (e <= abi.RTX_UPSAMPLE_E_MAX), np.exp(-np.where(cand, e, 0.0)), 0.0))
            wgt = np.where(fin, b * g, 0.0)
            m = np.ones((h, w, 3))
            if demodulate:
                both = (ap >= amin) & (aq >= amin) & (hit_p & hit_q)[..., None]
                m = np.where(both, ap / np.where(both, aq, 1.0), 1.0)
                if (wgt > 0).any():
                    R = max(R, float(m[wgt > 0].max()))
            num += wgt[..., None] * m * c
            den += wgt
    some = bden > 0
    bil = np.where(some[..., None], bnum / np.where(some, bden, 1.0)[..., None], 0.0)
    good = den > 0
    rgb = np.where(good[..., None], num / np.where(good, den, 1.0)[..., None], bil)
    conf = np.where(good, den / ball, 0.0)
    return {"rgb": rgb, "conf": conf, "bilinear": bil, "R": R, "margin": margin}


def tiles(conf, threshold):
    """the refinement list: the row-major indices of the 8x8 tiles with a pixel of conf < threshold (float32 compare)"""
    cf = np.asarray(conf, np.float32)
    h, w = cf.shape
    below = np.zeros((-(-h // 8) * 8, -(-w // 8) * 8), bool)
    below[:h, :w] = cf < np.float32(threshold)
    per_tile = below.reshape(below.shape[0] // 8, 8, below.shape[1] // 8, 8).any(axis=(1, 3))
    return np.flatnonzero(per_tile.reshape(-1)).astype(np.uint32)


def _fields(x, y, W, H):
    """the synthetic scene at continuous full-pixel coordinates: two surfaces that meet at the middle column (a flat one
    with a depth ramp, a curved one), a band of misses, a checkerboard of two materials whose albedo also varies
    smoothly, a lower band of two further materials of the SAME albedo, and a thin object 0.6 pixels wide at column 11
    that the low frames' pixel centres (s = 2, 3, 4) never meet"""
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
    alb = np.where(check[..., None], np.array([0.15, 0.2, 0.6]), np.array([0.9, 0.85, 0.8])) * (1 + 0.25 * np.sin(y / 3))[..., None]
    mat = check.astype(np.int32) + np.where(y >= 22, 2, 0)
    thin = (np.abs(x - 11) < 0.3) & (y >= 12) & (y < 20)
    z = np.where(thin, 3.0, z)
    n = np.where(thin[..., None], np.array([0.6, 0.0, -0.8]), n)
    alb = np.where(thin[..., None], np.array([0.4, 0.9, 0.3]), alb)
    mat = np.where(thin, 5, mat)
    obj = np.where(thin, 2, np.where(left, 0, 1))
    feat = np.zeros(x.shape, abi.FEATURE_DTYPE)
    feat["z"] = z
    feat["position"] = d * z[..., None]
    feat["normal"] = n
    feat["albedo"] = alb
    feat["material"] = mat
    feat["object"] = obj
    for f in ("z", "position", "normal", "albedo"):
        feat[f] = np.where(miss.reshape(miss.shape + (1,) * (feat[f].ndim - 2)), 0, feat[f])
    feat["material"][miss] = -1
    feat["object"][miss] = -1
    return feat


def synthetic(s=2, W=37, H=29):
    """(low_rgb (lh, lw, 3) float32, low_features (lh, lw), features (H, W)): the synthetic scene sampled at the full
    frame's pixels and at the centres of the low frame's s x s blocks, the low colour an albedo-shaded, noisy frame
    with one NaN and one inf"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    feat = _fields(x, y, W, H)
    lh, lw = low_size(H, s), low_size(W, s)
    ly, lx = np.mgrid[0:lh, 0:lw].astype(np.float64)
    lx, ly = lx * s + (s - 1) / 2, ly * s + (s - 1) / 2
    low = _fields(lx, ly, W, H)
    assert not (low["material"] == 5).any() and (feat["material"] == 5).any()
    shade = (0.6 + 0.3 * np.sin(lx / 5)) * np.where(low["material"] >= 2, 0.5, 1.0)
    rgb = low["albedo"].astype(np.float64) * shade[..., None] + np.abs(np.random.default_rng(5 + s).normal(0, 0.25, (lh, lw, 3)))
    rgb[low["z"] == 0] = 0.05
    rgb = rgb.astype(np.float32)
    rgb[2, 3, 1] = np.nan
    rgb[lh - 2, lw - 3, 0] = np.inf
    return rgb, low, feat


def finite_max(c):
    return float(np.abs(c[np.isfinite(c)]).max())
