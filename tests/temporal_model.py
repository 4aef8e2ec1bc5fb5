"""A float64 numpy model of the temporal accumulation (include/rtx.h rtx_frame_project, rtx_temporal*),
and the synthetic pair of frames test_gpu_temporal.py accumulates: an analytic scene that the model ray-casts itself
from two cameras.  The model gathers whole arrays per tap, so a small frame takes milliseconds."""
import numpy as np

from rtxpy import abi

SIGMAS = {"sigma_normal": 0.3, "sigma_albedo": 0.1, "sigma_plane": 0.02}
TERMS = ("normal", "albedo", "plane", "material", "length", "squared")
F32 = lambda x: float(np.float32(x))  # noqa: E731


def vec(v):
    return np.array(list(v), np.float32).astype(np.float64)


def make_frame(width, height, position, right, down, forward, pixel, focal=1.0):
    """an abi.Frame as rtx_frame_setup lays it out: the image plane `focal` in front of `position`, pixels `pixel` wide"""
    fr = abi.Frame()
    fr.width, fr.height = width, height
    position, right, down, forward = (np.asarray(a, np.float64) for a in (position, right, down, forward))
    sx, sy = right * pixel, down * pixel
    corner = position + forward * focal + sx * (0.5 - width / 2) + sy * (0.5 - height / 2)
    for name, val in (("corner", corner), ("step_x", sx), ("step_y", sy), ("origin", position)):
        for i in range(3):
            getattr(fr, name)[i] = val[i]
    return fr


def inverse(frame):
    """M = [step_x | step_y | corner - origin]^-1 by the adjugate, and the origin, in float64"""
    a, b, o = vec(frame.step_x), vec(frame.step_y), vec(frame.origin)
    c = vec(frame.corner) - o
    ab, bc, ca = np.cross(a, b), np.cross(b, c), np.cross(c, a)
    return np.stack([bc, ca, ab]) / (ab @ c), o


def project(frame, P):
    """the header's projection of the (..., 3) points P (read as float32): u, v float64, in_front bool"""
    M, o = inverse(frame)
    d = np.asarray(P, np.float32).astype(np.float64) - o
    with np.errstate(divide="ignore", invalid="ignore"):
        q = d @ M.T
        return q[..., 0] / q[..., 2] - 1.0, q[..., 1] / q[..., 2], q[..., 2] > 0


def finite_max(*arrays):
    return max(float(np.abs(a[np.isfinite(a)]).max()) for a in arrays)


def temporal(cur_frame, rgb, var, feat, prev_frame=None, hist_rgb=None, hist_var=None, hist_len=None, hist_feat=None,
             max_history=32, sigmas=SIGMAS, match_material=True, without=None):
    """the header's formulas in float64.  Returns a dict: rgb (h, w, 3), var (h, w, 3) or None, len (h, w), conf (h, w),
    u, v (the projections, NaN where a pixel is not live), and margin: the least of |e / E_MAX - 1| over the taps that
    only the cut decides and, unless the frames are bytewise equal, of the distance of a live pixel's u or v from an
    integer.  `without` names a term to leave out: normal, albedo, plane, material (the material match), length (n is
    divided by S, so lost weight does not shorten the history) or squared (H takes the weights, not their squares)."""
    h, w = feat.shape
    assert (cur_frame.width, cur_frame.height) == (w, h) and rgb.shape == (h, w, 3)
    c = rgb.astype(np.float64)
    Vc = None if var is None else var.astype(np.float64)
    hit = feat["z"] != 0
    live = hit & np.isfinite(c).all(-1)
    if Vc is not None:
        with np.errstate(invalid="ignore"):
            live &= (np.isfinite(Vc) & (Vc >= 0)).all(-1)
    out = {"rgb": c.copy(), "var": None if Vc is None else Vc.copy(), "len": np.where(live, 1.0, 0.0),
           "conf": np.where(hit, 0.0, 1.0), "margin": np.inf, "u": np.full((h, w), np.nan), "v": np.full((h, w), np.nan)}
    if prev_frame is None:
        return out
    assert (prev_frame.width, prev_frame.height) == (w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    if bytes(cur_frame) == bytes(prev_frame):
        u, v, front = xs.astype(np.float64), ys.astype(np.float64), np.ones((h, w), bool)
    else:
        u, v, front = project(prev_frame, feat["position"])
        fin = live & front & np.isfinite(u) & np.isfinite(v)
        if fin.any():
            out["margin"] = float(min(np.abs(u[fin] - np.round(u[fin])).min(), np.abs(v[fin] - np.round(v[fin])).min()))
    out["u"], out["v"] = np.where(live, u, np.nan), np.where(live, v, np.nan)
    with np.errstate(invalid="ignore"):
        reach = live & front & np.isfinite(u) & np.isfinite(v) & (u > -1) & (u < w) & (v > -1) & (v < h)
    us, vs = np.where(reach, u, 0.0), np.where(reach, v, 0.0)
    x0, y0 = np.floor(us).astype(np.int64), np.floor(vs).astype(np.int64)
    fx, fy = (us - x0).astype(np.float32), (vs - y0).astype(np.float32)
    inv = {t: 0.0 if t == without else 1.0 / F32(sigmas["sigma_" + t]) ** 2 for t in ("normal", "albedo", "plane")}
    zi, Pi, ni, ai = (feat[f].astype(np.float64) for f in ("z", "position", "normal", "albedo"))
    zi = np.where(hit, zi, 1.0)
    hc, L = hist_rgb.astype(np.float64), hist_len.astype(np.float64)
    Vh = None if hist_var is None else hist_var.astype(np.float64)
    S, n = np.zeros((h, w)), np.zeros((h, w))
    hs, Hs = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    one = np.float32(1)
    for b in (0, 1):
        for a in (0, 1):
            qx, qy = x0 + a, y0 + b
            bw = ((fx if a else one - fx) * (fy if b else one - fy)).astype(np.float64)  # the product in float32
            cons = reach & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h) & (bw > 0)
            Q = (np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1))
            t, Lq, gq = hc[Q], L[Q], hist_feat[Q]
            with np.errstate(invalid="ignore"):
                ok = cons & (Lq >= 1) & np.isfinite(Lq) & np.isfinite(t).all(-1) & (gq["z"] != 0)
                if Vh is not None:
                    ok &= (np.isfinite(Vh[Q]) & (Vh[Q] >= 0)).all(-1)
            if match_material and without != "material":
                ok &= feat["material"] == gq["material"]
            nq, aq, Pq = (gq[f].astype(np.float64) for f in ("normal", "albedo", "position"))
            with np.errstate(invalid="ignore", over="ignore"):
                e = (((ni - nq) ** 2).sum(-1) * inv["normal"] + ((ai - aq) ** 2).sum(-1) * inv["albedo"]
                     + (ni * (Pq - Pi)).sum(-1) ** 2 * inv["plane"] / zi ** 2)
            if ok.any():
                out["margin"] = min(out["margin"], float(np.nanmin(np.abs(e[ok] / abi.RTX_TEMPORAL_E_MAX - 1))))
            with np.errstate(invalid="ignore"):
                ok &= e <= abi.RTX_TEMPORAL_E_MAX
            wt = np.where(ok, bw * np.exp(-np.where(ok, e, 0.0)), 0.0)
            S += wt
            n += wt * np.where(ok, Lq, 0.0)
            hs += wt[..., None] * np.where(ok[..., None], t, 0.0)
            if Vh is not None:
                Hs += (wt if without == "squared" else wt * wt)[..., None] * np.where(ok[..., None], Vh[Q], 0.0)
    good = S > 0
    Sg = np.where(good, S, 1.0)
    if without == "length":
        n = n / Sg
    npr = np.minimum(n, max_history - 1.0)
    alpha = 1.0 / (npr + 1.0)
    hm = hs / Sg[..., None]
    cz = np.where(live[..., None], c, 0.0)
    out["rgb"] = np.where(good[..., None], hm + alpha[..., None] * (cz - hm), c)
    if Vc is not None:
        H = Hs / (Sg if without == "squared" else Sg * Sg)[..., None]
        Vz = np.where(live[..., None], Vc, 0.0)
        out["var"] = np.where(good[..., None], ((1 - alpha) ** 2)[..., None] * H + (alpha ** 2)[..., None] * Vz, Vc)
    out["len"] = np.where(good, npr + 1.0, out["len"])
    out["conf"] = np.where(good, S, out["conf"])
    return out


# ---- the synthetic pair ----
WALL_Z, RECT_Z, COL_Z = 6.0, 3.5, 4.0
PIXEL = 0.02          # the pixel's width on the image plane one unit in front of the camera
RECT = (-0.55, 0.05, -0.5, 0.1)   # world x0, x1, y0, y1 of the nearer rectangle
COL_X, COL_HALF, COL_Y = 0.262, 0.3 * PIXEL * COL_Z, (-0.4, 0.45)   # a column 0.6 pixels wide


def _cast(frame):
    """the records of the analytic scene seen through `frame`: a back wall at z = WALL_Z with a hole (misses) in one
    corner, two albedos that meet at world x = 0.9 and vary smoothly, two materials of the SAME albedo that meet at world
    y = 0.5 and a crease in its shading normal at world x = -1.2; a nearer rectangle of a material of its own; a column
    thinner than a pixel that differs from the wall behind it by its depth alone"""
    h, w = frame.height, frame.width
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    o = vec(frame.origin)
    d = vec(frame.corner) + ys[..., None] * vec(frame.step_y) + (xs[..., None] + 1) * vec(frame.step_x) - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)

    def plane(z):
        t = (z - o[2]) / d[..., 2]
        return t, o + d * t[..., None]

    t, P = plane(WALL_Z)
    obj = np.zeros((h, w), np.int32)
    miss = (P[..., 0] > 1.55) & (P[..., 1] < -0.9)
    for k, (z, inside) in enumerate(((RECT_Z, lambda Q: (Q[..., 0] > RECT[0]) & (Q[..., 0] < RECT[1]) & (Q[..., 1] > RECT[2]) & (Q[..., 1] < RECT[3])),
                                     (COL_Z, lambda Q: (np.abs(Q[..., 0] - COL_X) < COL_HALF) & (Q[..., 1] > COL_Y[0]) & (Q[..., 1] < COL_Y[1])))):
        tk, Pk = plane(z)
        m = inside(Pk)
        t, P, obj, miss = np.where(m, tk, t), np.where(m[..., None], Pk, P), np.where(m, k + 1, obj), miss & ~m
    X, Y = P[..., 0], P[..., 1]
    alb = np.where((X < 0.9)[..., None], np.array([0.9, 0.85, 0.8]), np.array([0.15, 0.2, 0.6])) * (1 + 0.2 * np.sin(3 * Y))[..., None]
    nrm = np.where((X < -1.2)[..., None], np.array([0.3, 0.0, -np.sqrt(1 - 0.09)]), np.array([0.0, 0.0, -1.0]))
    mat = (Y > 0.5).astype(np.int32)
    rect = obj == 1
    alb = np.where(rect[..., None], np.array([0.4, 0.9, 0.3]), alb)
    mat = np.where(rect, 2, mat)
    f = np.zeros((h, w), abi.FEATURE_DTYPE)
    f["position"], f["z"], f["normal"], f["albedo"], f["material"], f["object"] = P, t, nrm, alb, mat, obj
    for k in ("position", "z", "normal", "albedo"):
        f[k][miss] = 0
    f["material"][miss], f["object"][miss] = -1, -1
    return f


def synthetic(W=37, H=29):
    """a dict: prev_frame / cur_frame (the camera moved sideways and down by a few pixels of image shift and rolled by
    0.4 degrees), their records g / f rounded to float32, the current colour c and variance Vc, the history hc, Vh
    (one NaN and one inf each side of them) and the lengths L (integers 0..40, zeros included)"""
    prev = make_frame(W, H, (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), PIXEL)
    th = 0.007
    cur = make_frame(W, H, (-3.42 * PIXEL * WALL_Z, -1.27 * PIXEL * WALL_Z, 0), (np.cos(th), np.sin(th), 0), (-np.sin(th), np.cos(th), 0),
                     (0, 0, 1), PIXEL)
    g, f = _cast(prev), _cast(cur)
    rng = np.random.default_rng(11)
    c = (f["albedo"] * (0.5 + 0.4 * rng.random((H, W, 1))) + rng.random((H, W, 3)) * 0.2).astype(np.float32)
    hc = (g["albedo"] * (0.5 + 0.4 * rng.random((H, W, 1))) + rng.random((H, W, 3)) * 0.2).astype(np.float32)
    Vc = (rng.random((H, W, 3)) * 0.01).astype(np.float32)
    Vh = (rng.random((H, W, 3)) * 0.004).astype(np.float32)
    L = rng.integers(0, 41, (H, W)).astype(np.float32)
    L[rng.random((H, W)) < 0.05] = 0
    hc[5, 9, 1], hc[20, 30, 0] = np.nan, np.inf
    Vh[12, 12, 2], Vh[8, 25, 0] = np.nan, np.inf
    return dict(prev_frame=prev, cur_frame=cur, g=g, f=f, c=c, Vc=Vc, hc=hc, Vh=Vh, L=L)


def model_of(s, **kw):
    """the model on a synthetic() dict"""
    return temporal(s["cur_frame"], s["c"], s["Vc"], s["f"], s["prev_frame"], s["hc"], s["Vh"], s["L"], s["g"], **kw)


def shape_pair(w, h, seed=0):
    """a random pair for a w x h frame, as a synthetic() dict: one wall seen from two cameras, the current records'
    positions placed so that every pixel's (u, v) keeps 0.2 of a pixel away from the integers; two materials, smooth
    normals and albedos, a few misses on both sides"""
    rng = np.random.default_rng(w * 1000 + h * 10 + seed)
    prev = make_frame(w, h, (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), PIXEL)
    cur = make_frame(w, h, (-2.4 * PIXEL * WALL_Z, 1.3 * PIXEL * WALL_Z, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), PIXEL)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)

    def records(frame, ux, vy):
        """the wall's records at the frame's continuous pixel coordinates (ux, vy)"""
        o = vec(frame.origin)
        d = vec(frame.corner) + vy[..., None] * vec(frame.step_y) + (ux[..., None] + 1) * vec(frame.step_x) - o
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        t = (WALL_Z - o[2]) / d[..., 2]
        P = o + d * t[..., None]
        f = np.zeros((h, w), abi.FEATURE_DTYPE)
        f["position"], f["z"] = P, t
        f["normal"] = np.array([0, 0, -1.0]) + 0.1 * np.stack([np.sin(P[..., 0] * 5), np.cos(P[..., 1] * 5), 0 * t], -1)
        f["albedo"] = 0.4 + 0.05 * np.stack([np.sin(P[..., 0] * 9), np.cos(P[..., 1] * 7), np.sin(P[..., 0] + P[..., 1])], -1)
        f["material"] = np.sin(P[..., 0] * 4) > -0.6
        return f

    def with_misses(f):
        miss = rng.random((h, w)) < 0.1
        for k in ("z", "position", "normal", "albedo"):
            f[k][miss] = 0
        f["material"][miss], f["object"][miss] = -1, -1
        return f

    g = with_misses(records(prev, xs, ys))
    f = with_misses(records(cur, xs + 0.2 * (rng.random((h, w)) - 0.5), ys + 0.2 * (rng.random((h, w)) - 0.5)))
    c, hc = rng.random((h, w, 3), np.float32), rng.random((h, w, 3), np.float32)
    Vc, Vh = rng.random((h, w, 3), np.float32) * 0.01, rng.random((h, w, 3), np.float32) * 0.01
    L = rng.integers(0, 41, (h, w)).astype(np.float32)
    return dict(prev_frame=prev, cur_frame=cur, g=g, f=f, c=c, Vc=Vc, hc=hc, Vh=Vh, L=L)
