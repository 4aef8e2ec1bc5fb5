"""A numpy float64 model of rtx_projection's camera models, written from the formulas in include/rtx.h (not from
the library's C++), and the comparison rule the projection tests share.

    r = unit(step_x), dn = unit(step_y), f = +-(r x dn) with f . (corner + (W/2) step_x + (H/2) step_y - origin) > 0
    u = (px + 1/2 + offset_x) / W,  v = (py + 1/2 + offset_y) / H
    panorama  lambda = (u - 1/2) fov, phi = (1/2 - v) pi (fov / 2 pi) (2 H / W); |phi| > pi/2 a hole
              d = cos phi (sin lambda r + cos lambda f) - sin phi dn
    fisheye   x = 2u - 1, y = (2v - 1) H / W, rho = sqrt(x^2 + y^2), theta = rho fov / 2; theta > pi a hole
              d = cos theta f + sin theta (x r + y dn) / rho, d = f at rho = 0
    ortho     d = f, origin += (u - 1/2) E r + (v - 1/2) E (H / W) dn, E = extent or W |step_x|
"""
import numpy as np

from rtxpy import abi


def basis(frame):
    """(r, dn, f, origin) in float64 of an abi.Frame"""
    sx, sy = np.array(frame.step_x[:], np.float64), np.array(frame.step_y[:], np.float64)
    corner, origin = np.array(frame.corner[:], np.float64), np.array(frame.origin[:], np.float64)
    r, dn = sx / np.sqrt(sx @ sx), sy / np.sqrt(sy @ sy)
    f = np.cross(r, dn)
    f /= np.sqrt(f @ f)
    centre = corner + (frame.width / 2.0) * sx + (frame.height / 2.0) * sy
    if f @ (centre - origin) < 0:
        f = -f
    return r, dn, f, origin


def rays(frame, proj):
    """the model's rays: (origin (h, w, 3), dir (h, w, 3)) float64 and hole (h, w) bool"""
    W, H = frame.width, frame.height
    r, dn, f, o = basis(frame)
    py, px = np.mgrid[0:H, 0:W].astype(np.float64)
    u = (px + 0.5 + np.float64(proj.offset_x)) / W
    v = (py + 0.5 + np.float64(proj.offset_y)) / H
    fov, E = np.float64(proj.fov), np.float64(proj.extent)
    origin = np.broadcast_to(o, (H, W, 3)).copy()
    hole = np.zeros((H, W), bool)
    if proj.kind == abi.RTX_PROJ_PANORAMA:
        lam = (u - 0.5) * fov
        phi = (0.5 - v) * np.pi * (fov / (2.0 * np.pi)) * (2.0 * H / W)
        hole = np.abs(phi) > np.pi / 2.0
        d = (np.cos(phi)[..., None] * (np.sin(lam)[..., None] * r + np.cos(lam)[..., None] * f)
             - np.sin(phi)[..., None] * dn)
    elif proj.kind == abi.RTX_PROJ_FISHEYE:
        x, y = 2.0 * u - 1.0, (2.0 * v - 1.0) * H / W
        rho = np.sqrt(x * x + y * y)
        theta = rho * fov / 2.0
        hole = theta > np.pi
        safe = np.where(rho == 0.0, 1.0, rho)
        d = (np.cos(theta)[..., None] * f
             + np.sin(theta)[..., None] * (x[..., None] * r + y[..., None] * dn) / safe[..., None])
        d[rho == 0.0] = f
    elif proj.kind == abi.RTX_PROJ_ORTHO:
        if E == 0.0:
            sx = np.array(frame.step_x[:], np.float64)
            E = W * np.sqrt(sx @ sx)
        d = np.broadcast_to(f, (H, W, 3)).copy()
        origin = o + ((u - 0.5) * E)[..., None] * r + ((v - 0.5) * E * (H / W))[..., None] * dn
    else:
        raise ValueError(proj.kind)
    return origin, d, hole


def compare(records, frame, proj):
    """records: (h, w) of abi.RAY_DTYPE against the model: the holes identical (all-zero records), every other ray with
    tmax = inf and each component within one float32 ulp of the model's value rounded to float32.  Returns the
    number of components that differ at all and the number compared."""
    origin, d, hole = rays(frame, proj)
    rec = np.asarray(records).reshape(frame.height, frame.width)
    assert np.array_equal(rec["tmax"] <= 0, hole)
    holes = rec[hole]
    for k in ("origin", "tmax", "dir", "pad_"):
        assert not np.any(holes[k])
    assert np.all(np.isinf(rec["tmax"][~hole])) and not np.any(rec["pad_"])
    differ = total = 0
    for got, want in ((rec["origin"], origin), (rec["dir"], d)):
        g, w32 = got[~hole], want[~hole].astype(np.float32)
        err = np.abs(g.astype(np.float64) - w32.astype(np.float64))
        assert np.all(err <= np.spacing(np.abs(w32)).astype(np.float64)), float(err.max())
        differ += int(np.count_nonzero(g != w32))
        total += g.size
    return differ, total
