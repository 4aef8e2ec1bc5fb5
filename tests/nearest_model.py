"""A float64 model of the closest-point queries' definition and the point families of their tests
(test_nearest_model.py on the CPU, test_gpu_nearest.py on the GPU).

The model restates csrc/rtx_nearest_math.h in plain numpy float64 on the scene's float32 records: the
triangle p0, p0 + e1, p0 + e2 by the closest points of its three edge segments and the foot of the
perpendicular where it lies in the triangle, the sphere and the plane by their formulas.  float32's
answer is held to it in units of one float32 ulp of the largest coordinate magnitude among the point and
the object (cancellation error scales with the coordinates, not with dist).
"""
import numpy as np

import hard_meshes as HM
import rays_exhaustive as RX
from rtxpy import abi

# The largest error of dist over the fixtures of test_nearest_model.py, in those ulps, as measured on the
# development host, and the asserted bound: 4 times it (the factor covers points the fixtures do not reach).
DIST_ULPS_OBSERVED = 5.2  # 5.16, on count1024
DIST_ULPS_BOUND = 4 * DIST_ULPS_OBSERVED

N_POINTS = 1024  # per family of the search tests


# ---- the model ----
def _segment(ap, ab):
    l2 = (ab * ab).sum(1)
    t = np.where(l2 > 0, (ap * ab).sum(1) / np.where(l2 > 0, l2, 1.0), 0.0)
    return np.clip(t, 0.0, 1.0)[:, None] * ab


def model(objs, P):
    """pair i: object record objs[i] and point P[i]; float64 (dist (n,), cp (n, 3))"""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    n = len(P)
    assert len(objs) == n
    dist, cp = np.zeros(n), np.zeros((n, 3))
    typ = objs["type"]
    t = np.nonzero(typ == abi.RTX_TRIANGLE)[0]
    if len(t):
        p0, e1, e2 = (objs[k][t].astype(np.float64) for k in ("p0", "e1", "e2"))
        ap = P[t] - p0
        cand = [_segment(ap, e1), _segment(ap, e2), e1 + _segment(ap - e1, e2 - e1)]
        d11, d12, d22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
        b1, b2 = (ap * e1).sum(1), (ap * e2).sum(1)
        det = d11 * d22 - d12 * d12
        ok = det > 0
        sd = np.where(ok, det, 1.0)
        v, w = (d22 * b1 - d12 * b2) / sd, (d11 * b2 - d12 * b1) / sd
        inside = ok & (v >= 0) & (w >= 0) & (v + w <= 1)
        face = v[:, None] * e1 + w[:, None] * e2
        d2 = np.stack([((ap - q) ** 2).sum(1) for q in cand] + [np.where(inside, ((ap - face) ** 2).sum(1), np.inf)])
        k = d2.argmin(0)
        q = np.stack(cand + [face])[k, np.arange(len(t))]
        dist[t] = np.sqrt(d2.min(0))
        cp[t] = p0 + q
    s = np.nonzero(typ == abi.RTX_SPHERE)[0]
    if len(s):
        c, r = objs["p0"][s].astype(np.float64), objs["radius"][s].astype(np.float64)
        d = P[s] - c
        l = np.sqrt((d * d).sum(1))
        dist[s] = np.abs(l - r)
        cp[s] = np.where((l > 0)[:, None], c + d * (r / np.where(l > 0, l, 1.0))[:, None], c + np.stack([r, 0 * r, 0 * r], 1))
    p = np.nonzero(typ == abi.RTX_PLANE)[0]
    if len(p):
        nn, dd = objs["n"][p].astype(np.float64), objs["d"][p].astype(np.float64)
        sgn = (nn * P[p]).sum(1) - dd
        dist[p] = np.abs(sgn)
        cp[p] = P[p] - sgn[:, None] * nn
    return dist, cp


def coord_ulp(objs, P):
    """pair i: one float32 ulp of the largest coordinate magnitude among the point and the object's vertices
    (a sphere's centre and radius, a plane's offset d)"""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    p0, e1, e2 = (objs[k].astype(np.float64) for k in ("p0", "e1", "e2"))
    tri = (objs["type"] == abi.RTX_TRIANGLE)[:, None]
    sph = objs["type"] == abi.RTX_SPHERE
    m = np.abs(P).max(1)
    m = np.maximum(m, np.where(objs["type"] == abi.RTX_PLANE, np.abs(objs["d"].astype(np.float64)), np.abs(p0).max(1)))
    m = np.maximum(m, np.where(tri, np.maximum(np.abs(p0 + e1), np.abs(p0 + e2)), 0.0).max(1))
    m = np.maximum(m, np.where(sph, np.abs(objs["radius"].astype(np.float64)), 0.0))
    return np.spacing(m.astype(np.float32)).astype(np.float64)


def segment_distance(objs, X):
    """pair i: the float64 distance from X[i] to the longest edge segment of triangle objs[i] (the segment a
    zero-area triangle collapses to; a point when every edge is zero)"""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    p0, e1, e2 = (objs[k].astype(np.float64) for k in ("p0", "e1", "e2"))
    segs = [(p0, e1), (p0, e2), (p0 + e1, e2 - e1)]
    l2 = np.stack([(ab * ab).sum(1) for _, ab in segs])
    k = l2.argmax(0)
    a = np.stack([a for a, _ in segs])[k, np.arange(len(X))]
    ab = np.stack([ab for _, ab in segs])[k, np.arange(len(X))]
    q = a + _segment(X - a, ab)
    return np.sqrt(((X - q) ** 2).sum(1))


def host(objs, idx, P):
    """rtx_closest_point_object on the pairs (objs[idx[i]], P[i]): float32 (dist (n,), cp (n, 3))"""
    import ctypes
    import rtxpy
    fn = rtxpy.rtx_lib().rtx_closest_point_object
    objs = np.ascontiguousarray(objs)
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3)
    out = np.zeros((len(P), 4), np.float32)
    base, size = objs.ctypes.data, objs.dtype.itemsize
    pp, po = P.ctypes.data, out.ctypes.data
    for i, o in enumerate(np.asarray(idx).tolist()):
        rc = fn(base + o * size, pp + 12 * i, po + 16 * i, po + 16 * i + 4)
        assert rc == 0, (i, o, rc)
    return out[:, 0].copy(), out[:, 1:].copy()


def pairs_of(objs, seed=9):
    """the (object row, point) pairs the arithmetic is checked on: every family of object_points on a sample of the
    scene's objects, each point against its own object and against another one of the sample, and the free
    families against objects of the sample"""
    rs = np.random.RandomState(seed)
    rows = sample_objects(objs)
    if not len(rows):
        return np.zeros(0, np.int64), np.zeros((0, 3), np.float32)
    who, pts = object_points(objs, rows)
    idx, P = [who, rows[rs.randint(len(rows), size=len(who))]], [pts, pts]
    for v in free_points(objs, 256).values():
        idx.append(rows[rs.randint(len(rows), size=len(v))])
        P.append(v)
    # the spheres and the planes are few: 1024 more pairs for each type the scene has, on points of every family
    allp = np.concatenate(P)
    for t in (abi.RTX_SPHERE, abi.RTX_PLANE):
        of = np.nonzero(objs["type"] == t)[0]
        if len(of):
            idx.append(of[rs.randint(len(of), size=1024)])
            P.append(allp[rs.randint(len(allp), size=1024)])
    return np.concatenate(idx), np.concatenate(P)


# ---- point families ----
def _unit(rs, n):
    v = rs.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _verts(objs):
    p0, e1, e2 = (objs[k].astype(np.float64) for k in ("p0", "e1", "e2"))
    return p0, p0 + e1, p0 + e2


def _box(objs):
    lo, hi = HM._box(objs)
    return np.asarray(lo, np.float64), np.asarray(hi, np.float64)


def object_points(objs, rows, seed=5):
    """the point families tied to single objects, for the objects `rows`: (object row (m,), points (m, 3) float32).
    Triangles: vertices, edge midpoints, the centroid, and each of those displaced along the normal (any unit vector
    for a zero-area triangle) by 1e-6, 1e-3 and 1 box diagonals; spheres: the centre, points on the surface, the same
    displacements along the radius."""
    rs = np.random.RandomState(seed)
    lo, hi = _box(objs)
    diag = float(np.linalg.norm(hi - lo))
    o = objs[rows]
    a, b, c = _verts(o)
    who, pts = [], []
    tri = np.nonzero(o["type"] == abi.RTX_TRIANGLE)[0]
    if len(tri):
        base = [a[tri], b[tri], c[tri], 0.5 * (a[tri] + b[tri]), 0.5 * (b[tri] + c[tri]), 0.5 * (c[tri] + a[tri]),
                (a[tri] + b[tri] + c[tri]) / 3.0]
        nrm = np.cross(b[tri] - a[tri], c[tri] - a[tri])
        ln = np.linalg.norm(nrm, axis=1, keepdims=True)
        nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), _unit(rs, len(tri)))
        for x in base:
            who.append(rows[tri])
            pts.append(x)
        for x in (base[0], base[3], base[6]):
            for s in (1e-6, 1e-3, 1.0, -1e-3):
                who.append(rows[tri])
                pts.append(x + s * diag * nrm)
    sph = np.nonzero(o["type"] == abi.RTX_SPHERE)[0]
    if len(sph):
        cen, r = a[sph], o["radius"][sph].astype(np.float64)[:, None]
        u = _unit(rs, len(sph))
        for x in (cen, cen + r * u, cen + 0.5 * r * u):
            who.append(rows[sph])
            pts.append(x)
        for s in (1e-6, 1e-3, 1.0):
            who.append(rows[sph])
            pts.append(cen + (r + s * diag) * u)
    if not who:
        return np.zeros(0, np.int64), np.zeros((0, 3), np.float32)
    return np.concatenate(who), np.concatenate(pts).astype(np.float32)


def free_points(objs, n, seed=6):
    """the families tied to no object: {name: (n, 3) float32}: uniform in the bounded objects' box (widened by a
    tenth), and at 60 and 2000 radii from its centre"""
    rs = np.random.RandomState(seed)
    lo, hi = _box(objs)
    cen, rad = 0.5 * (lo + hi), 0.5 * float((hi - lo).max())
    ext = 0.55 * (hi - lo)
    out = {"inbox": cen + rs.uniform(-1, 1, size=(n, 3)) * ext}
    for k in (60, 2000):
        out["far%d" % k] = cen + k * rad * _unit(rs, n)
    return {k: v.astype(np.float32) for k, v in out.items()}


def search_families(objs, n=N_POINTS, seed=7):
    """the search tests' families, {name: (m, 3) float32}, m = n (`centre`: at most n, 0 without spheres):
    inbox / far60 / far2000 as free_points; surface: points on random bounded objects; vertex: triangle vertices;
    ties: points equidistant between faces (off a shared vertex along the ray from a face's centroid, where the
    vertex is the closest point of every face that shares it; and midway between two surface points); centre: the
    spheres' centres, exactly and displaced by 1e-7 .. 1e-2 radii."""
    rs = np.random.RandomState(seed)
    fam = free_points(objs, n, seed)
    b = np.nonzero(HM.is_bounded(objs))[0]
    if not len(b):
        z = np.zeros((0, 3), np.float32)
        fam.update(surface=z, vertex=z, ties=z, centre=z)
        return fam

    def surface(m):
        o = objs[rs.choice(b, m)]
        a, v1, v2 = _verts(o)
        u, v = rs.uniform(size=(2, m))
        flip = u + v > 1
        u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
        x = a + u[:, None] * (v1 - a) + v[:, None] * (v2 - a)
        sp = o["type"] == abi.RTX_SPHERE
        return np.where(sp[:, None], a + o["radius"].astype(np.float64)[:, None] * _unit(rs, m), x)

    fam["surface"] = surface(n).astype(np.float32)
    t = b[objs["type"][b] == abi.RTX_TRIANGLE]
    if len(t):
        o = objs[rs.choice(t, n)]
        vs = np.stack(_verts(o), 1)
        k = rs.randint(3, size=n)
        vert = vs[np.arange(n), k]
        fam["vertex"] = vert.astype(np.float32)
        out = vert - vs.mean(1)
        corner = vert.astype(np.float32).astype(np.float64) + out * rs.uniform(0.01, 0.5, size=(n, 1))
        mid = 0.5 * (surface(n) + surface(n))
        fam["ties"] = np.where((np.arange(n) % 2 == 0)[:, None], corner, mid).astype(np.float32)
    else:
        fam["vertex"] = np.zeros((0, 3), np.float32)
        fam["ties"] = (0.5 * (surface(n) + surface(n))).astype(np.float32)
    s = b[objs["type"][b] == abi.RTX_SPHERE]
    if len(s):
        m = min(n, 64 * len(s))
        o = objs[s[np.arange(m) % len(s)]]
        scale = np.where(np.arange(m) < len(s), 0.0, 10.0 ** rs.uniform(-7, -2, size=m))
        fam["centre"] = (o["p0"].astype(np.float64) + (scale * o["radius"])[:, None] * _unit(rs, m)).astype(np.float32)
    else:
        fam["centre"] = np.zeros((0, 3), np.float32)
    return fam


def sample_objects(objs, cap=192, seed=8):
    """rows of at most `cap` objects: every sphere, plane and zero-area triangle (up to cap / 2 of them), the rest
    drawn at random"""
    rs = np.random.RandomState(seed)
    special = np.nonzero((objs["type"] != abi.RTX_TRIANGLE) | HM.zero_area(objs))[0][:cap // 2]
    rest = np.setdiff1d(np.arange(len(objs)), special)
    take = rs.choice(rest, min(len(rest), cap - len(special)), replace=False) if len(rest) else rest
    return np.sort(np.concatenate([special, take])).astype(np.int64)


def scene_paths(tmp):
    """every fixture scene under `tmp`: the hard meshes and both exhaustive scenes, {name: (path, loader)}"""
    out = {name: (path, lambda p, name=name: HM.load(name, p)) for name, path in HM.write_scenes(tmp).items()}
    out.update({name: (path, RX.load) for name, path in RX.write_scenes(tmp).items()})
    return out
