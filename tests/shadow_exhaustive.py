"""Scenes, shadow-ray families and the expected answers of the exhaustive shadow-query tests
(test_shadow_exhaustive.py on the CPU, test_gpu_shadow_exhaustive.py on the GPU).

A shadow ray (origin, direction, dist, light object) is answered by k_shadow's own shadow_query
(rtx_trace_shadow_rays).  Its expected answer is brute force: over every object float32 could
conceivably accept (the candidates of rays_exhaustive.reference), the device's own any-hit tests
(rtx_kat: KAT_ANY_TRI with tlim = dist, KAT_SPHERE with t < dist) decide the triangles and spheres,
float64 decides the planes (the families keep every ray clear of a plane's thresholds), the light
object is left out, and

    blocked        = some opaque object is hit
    transmittance  = (2^-a, 2^-b, 2^-c) with a, b, c the hits of the transparent materials A, B, C

The transparent materials' kt are (0.5, 1, 1), (1, 0.5, 1) and (1, 1, 0.5): powers of two, so the
product is exact in any order and a dropped or doubled test changes the bits.

The families are made decisive by float64 geometry before anything is compared (_settle: a ray too
nearly parallel to a plane, or a far ray grazing a sphere, gives way to its neighbour), so no ray
and no (ray, object) pair is left out of a comparison.
"""
import json
import os

import numpy as np

import rays_exhaustive as RX
from rtxpy import abi

# materials: the template's 0 (sponge), 1 (emitter, opaque) and 2 (dragon) keep their numbers
# (rays_exhaustive tells the meshes apart by them); 3 is C, 4 opaque grey
MAT_C, MAT_GREY = 3, 4
KT = {"A": [0.5, 1.0, 1.0], "B": [1.0, 0.5, 1.0], "C": [1.0, 1.0, 0.5]}
SCENES = ("glass", "mixed", "trionly", "tiny")
VARIANTS = tuple(RX.ROTATION)
N_RAYS = RX.N_RAYS
MAX_EXPONENT = 100
SPHERE_CLEAR = 1e-3  # as test_gpu_rays_exhaustive.py: a ray this far inside the silhouette meets any box of the sphere


def _materials(tpl, scene):
    m = json.loads(json.dumps(tpl["Materials"]))
    grey = json.loads(json.dumps(m[2]))
    m += [json.loads(json.dumps(grey)), json.loads(json.dumps(grey))]
    m[3]["id"], m[4]["id"] = MAT_C, MAT_GREY
    for k in (0, 2, 3, 4):
        m[k]["kt"] = [0.0, 0.0, 0.0]
    m[RX.SPONGE_MAT]["kt"] = KT["A"]
    if scene in ("glass", "tiny"):
        m[RX.DRAGON_MAT]["kt"] = KT["B"]
    m[MAT_C]["kt"] = KT["C"]
    return m


def _lights():
    """one sphere light and one triangle light: opaque emitters, left out of the 8-wide tree"""
    return [{"type": "Sphere", "parameters": {"material": 1, "epsilon": 0.0003, "position": [0.4, 1.6, 1.5], "radius": 0.3,
                                              "lights": 4}},
            {"type": "Triangle", "parameters": {"material": 1, "vertex_1": [-1.9, 2.1, 1.6], "vertex_2": [-0.9, 2.1, 1.4],
                                                "vertex_3": [-1.5, 2.3, 2.6], "lights": 4}}]


def _plane(mat, pos, nrm):
    return {"type": "Plane", "parameters": {"material": mat, "epsilon": 0.00025, "position": pos, "normal": nrm}}


def _objects(scene, name):
    sphere = lambda mat: {"type": "Sphere", "parameters": {"material": mat, "position": [-1.6, 0.4, 2.2], "radius": 0.6}}
    back, floor = [0.0, 0.0, 8.0], [0.0, -1.5, 0.0]
    if scene == "glass":
        return RX.mesh_objects(name) + [sphere(MAT_C)] + _lights() + [_plane(MAT_C, floor, [0.0, 1.0, 0.0])]
    if scene in ("mixed", "trionly"):
        return (RX.mesh_objects(name) + ([sphere(MAT_GREY)] if scene == "mixed" else []) + _lights()
                + [_plane(MAT_GREY, back, [0.0, 0.0, 1.0]), _plane(MAT_C, floor, [0.0, 1.0, 0.0])])
    # tiny: six bounded objects (a transparent and an opaque triangle and sphere, the two lights) and both planes
    rot = RX.ROTATION[name]
    return [RX.mesh("tri_a.stl", RX.SPONGE_MAT, rot, 1.0, [0.0, 0.0, 2.4]), RX.mesh("tri_o.stl", MAT_GREY, rot, 1.0, [0.3, 0.2, 3.0]),
            sphere(MAT_C), {"type": "Sphere", "parameters": {"material": MAT_GREY, "position": [1.5, -0.4, 2.6], "radius": 0.5}}
            ] + _lights() + [_plane(MAT_GREY, back, [0.0, 0.0, 1.0]), _plane(MAT_C, floor, [0.0, 1.0, 0.0])]


def write_scenes(tmp):
    """every scene in both variants under `tmp`: {(scene, variant): path of its JSON}"""
    import standins
    tmp = str(tmp)
    tpl = RX.write_meshes(tmp)
    standins.write_stl(os.path.join(tmp, "meshes", "tri_a.stl"), np.array([[[-1.0, -0.8, 0.0], [1.1, -0.7, 0.1], [0.1, 1.0, -0.1]]], np.float32))
    standins.write_stl(os.path.join(tmp, "meshes", "tri_o.stl"), np.array([[[-0.7, -0.9, 0.1], [0.9, -0.2, 0.0], [-0.2, 0.8, 0.2]]], np.float32))
    out = {}
    for scene in SCENES:
        for name in VARIANTS:
            d = json.loads(json.dumps(tpl))
            d["Materials"] = _materials(tpl, scene)
            d["Objects"] = _objects(scene, name)
            out[scene, name] = os.path.join(tmp, "%s_%s.json" % (scene, name))
            with open(out[scene, name], "w") as fh:
                json.dump(d, fh)
    return out


class Mats:
    """per object of a scene: transparent, and which of A / B / C its material's kt is (-1: opaque)"""

    def __init__(self, scene, objs):
        n = scene.desc.num_materials
        kt = np.array([list(scene.desc.materials[i].kt[:]) for i in range(n)], np.float32)
        tr = np.array([scene.desc.materials[i].transparent != 0 for i in range(n)])
        which = np.full(n, -1)
        for k, key in enumerate("ABC"):
            which[(kt == np.array(KT[key], np.float32)).all(1)] = k
        assert (tr == (which >= 0)).all()  # every transparent material is one of the three
        self.channel = which[objs["material"]]
        self.transparent = self.channel >= 0


# ---- ray families ----
FAMILIES = ("light", "incoherent", "surface", "axis", "onezero", "edges", "onplane", "through", "far60", "idle")
FROM_RX = ("incoherent", "surface", "axis", "onezero", "edges", "onplane")
IDLE_SIZES = (1, 63, 65)  # further idle batches: the first rays of the family


class Rays:
    """a batch: origins o, unit directions d (float32 (n, 3)), dist (float32), light object (int32, -1: none),
    idle (the rays the entry must treat as idle lanes) and target_far (light family: the target lies on
    the emitter's far side)"""

    def __init__(self, o, d, dist, light=None, idle=None, target_far=None):
        n = len(o)
        self.o, self.d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        self.dist = np.ascontiguousarray(dist, np.float32)
        self.light = np.full(n, -1, np.int32) if light is None else np.ascontiguousarray(light, np.int32)
        self.idle = np.zeros(n, bool) if idle is None else idle
        self.target_far = np.zeros(n, bool) if target_far is None else target_far
        self.n = n

    def take(self, idx):
        return Rays(self.o[idx], self.d[idx], self.dist[idx], self.light[idx], self.idle[idx], self.target_far[idx])

    def without_light(self):
        return Rays(self.o, self.d, self.dist, None, self.idle, self.target_far)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _own_axes(objs, name):
    """the sponge's own axes (its face normals) in the rotated variant, else the world's"""
    if name != "rotated":
        return np.eye(3)
    tri = objs[objs["type"] == abi.RTX_TRIANGLE]
    own = []
    for v3 in tri[tri["material"] == RX.SPONGE_MAT]["n"].astype(np.float64):
        if all(abs(abs(v3 @ w) - 1) > 1e-3 for w in own):
            own.append(v3)
    assert len(own) == 3
    return np.array(own)


def _light_family(rs, objs, lo, hi):
    tri = objs[objs["type"] == abi.RTX_TRIANGLE]
    tri = tri[tri["num_lights"] == 0]
    emit = np.nonzero(objs["num_lights"] > 0)[0]
    assert len(emit) == 2
    floor = objs[(objs["type"] == abi.RTX_PLANE) & (np.abs(objs["n"][:, 1]) == 1)][0]
    o, d, dist, light, tfar = [], [], [], [], []
    for k in range(N_RAYS // 64):
        if k % 4 == 3:  # on the floor plane, under the scene
            p = np.array([rs.uniform(lo[0], hi[0]), float(floor["d"]) * float(floor["n"][1]), rs.uniform(lo[2], hi[2])])
        else:
            t = tri[rs.randint(0, len(tri))]
            u, v = rs.uniform(size=2)
            if u + v > 1:
                u, v = 1 - u, 1 - v
            p = t["p0"] + u * t["e1"].astype(np.float64) + v * t["e2"].astype(np.float64) + 1e-3 * t["n"].astype(np.float64)
        p = p.astype(np.float32).astype(np.float64)
        e = objs[emit[k % 2]]
        if e["type"] == abi.RTX_SPHERE:
            w = _unit(rs.normal(size=(64, 3)))
            target = e["p0"].astype(np.float64) + float(e["radius"]) * w
            far = (w * (e["p0"].astype(np.float64) - p)).sum(1) > 0.05 * np.linalg.norm(e["p0"] - p)
        else:
            u, v = rs.uniform(size=64), rs.uniform(size=64)
            fold = u + v > 1
            u[fold], v[fold] = 1 - u[fold], 1 - v[fold]
            target = e["p0"] + u[:, None] * e["e1"].astype(np.float64) + v[:, None] * e["e2"].astype(np.float64)
            far = np.zeros(64, bool)
        v = target - p
        o.append(np.repeat(p[None], 64, 0))
        d.append(_unit(v))
        dist.append(np.linalg.norm(v, axis=1))
        light.append(np.full(64, emit[k % 2]))
        tfar.append(far)
    return Rays(np.concatenate(o), np.concatenate(d), np.concatenate(dist), np.concatenate(light), None, np.concatenate(tfar))


# Body-diagonal lines of a level-2 Menger sponge that cross its surface 12 times: with the cube as [-1, 1]^3 and
# the line along (1, 1, 1) through a (1, -1, 0) / sqrt 2 + b (1, 1, -2) / sqrt 6, the offsets (a, b) within
# about 0.02 of the six points at radius 0.205 and angles k * 60 degrees (found by counting crossings on a
# 0.02 grid of offsets; the cube's reflections carry them to the other diagonals).  Axis and face-diagonal
# lines cross it 8 times at most, so without these no ray would gather a dozen transparent hits.
DENSE_RADIUS, DENSE_JITTER = 0.205, 0.012


def _through_family(rs, objs, name):
    """rays through the whole sponge along its own axes: half of them axis (a quarter of these) and
    diagonal rays from uniform points, half the body diagonals above"""
    tri = objs[objs["type"] == abi.RTX_TRIANGLE]
    sp = tri[tri["material"] == RX.SPONGE_MAT]
    ax = _own_axes(objs, name)
    pts = np.concatenate([sp["p0"], sp["p1"], sp["p2"]]).astype(np.float64) @ ax.T  # in the sponge's frame
    lo, hi = pts.min(0), pts.max(0)
    ce, he = 0.5 * (lo + hi), 0.5 * (hi - lo)
    n = N_RAYS // 2
    sgn = lambda m: np.where(rs.randint(0, 2, size=m) == 1, 1.0, -1.0)
    kind = rs.randint(0, 4, size=n)  # 0: axis, 1: face diagonal, 2 and 3: body diagonal
    dl = np.stack([sgn(n), sgn(n), sgn(n)], 1)
    drop = rs.randint(0, 3, size=n)
    for k in range(3):
        dl[(kind == 0) & (drop != k), k] = 0.0
        dl[(kind == 1) & (drop == k), k] = 0.0
    dl = _unit(dl)
    p = rs.uniform(lo, hi, size=(n, 3))
    # the dense body diagonals
    ang = rs.randint(0, 6, size=n) * (np.pi / 3)
    a = DENSE_RADIUS * np.cos(ang) + rs.uniform(-DENSE_JITTER, DENSE_JITTER, size=n)
    b = DENSE_RADIUS * np.sin(ang) + rs.uniform(-DENSE_JITTER, DENSE_JITTER, size=n)
    U, V = np.array([1.0, -1.0, 0.0]) / np.sqrt(2), np.array([1.0, 1.0, -2.0]) / np.sqrt(6)
    mirror = np.stack([sgn(n), sgn(n), sgn(n)], 1)  # a reflection of the cube and the ray's sense
    pd = ce + he * mirror * (a[:, None] * U + b[:, None] * V)
    dd = _unit(mirror * sgn(n)[:, None])
    p, dl = np.concatenate([p, pd]), np.concatenate([dl, dd])
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    back = ((p[:, None, :] - corners[None]) * dl[:, None, :]).sum(-1).max(1) + 0.5
    ol = p - dl * back[:, None]
    return ol @ ax, dl @ ax


def _far_family(rs, lo, hi, rad):
    """origins 60 radii out, aimed at uniform points of the bounded objects' box"""
    target = rs.uniform(lo, hi, size=(N_RAYS, 3))
    d = RX._sphere_dirs(rs, N_RAYS)
    return target - 60.0 * rad * d, d


def plane_view(objs, o, d, dist):
    """float64 on the float32 records (rtx_math.h hit_plane, then t < dist), per (ray, plane): hit, and
    where float32 might decide otherwise: |n.d| within [eps / 2, 2 eps] or t within 1e-4 of eps
    (shaky), t within 1e-4 of dist (short)"""
    pl = np.nonzero(objs["type"] == abi.RTX_PLANE)[0]
    o, d, dist = (np.asarray(x).astype(np.float64) for x in (o, d, dist))
    nn, dd, eps = (objs[c][pl].astype(np.float64) for c in ("n", "d", "epsilon"))
    a = d @ nn.T
    absa = np.abs(a)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (dd[None] - o @ nn.T) / a
        hit = (absa >= eps[None]) & (t > eps[None]) & (t < dist[:, None])
        shaky = ((absa >= 0.5 * eps[None]) & (absa <= 2 * eps[None])) | ((absa > 2 * eps[None]) & (np.abs(t - eps[None]) <= 1e-4 * eps[None]))
        short = (absa > 2 * eps[None]) & (np.abs(t - dist[:, None]) <= 1e-4 * dist[:, None])
    return pl, hit, shaky, short


# a far ray's geometric discriminant over r^2 in here: hit_sphere's own b * b - c cancels.  From 60
# radii |o - c| is about 200, so float32 rounds the two terms by about 4 * 2^-24 * 200^2 = 1e-2 together: 0.1 of the
# smaller sphere's r^2 = 0.09
GRAZE = (-0.1, 2 * SPHERE_CLEAR)


def _settle(objs, r, far):
    """the family made decisive, by float64 geometry alone: a ray nearly parallel to a plane or starting
    a plane's epsilon from it (and, of a far family, one that grazes a sphere, where the far-sphere
    exception of DESIGN §7.3 would apply) is replaced by the nearest ray of its 64-ray packet that is
    not; a dist within 1e-4 of a plane's t is shortened by 3 %.  Every ray left is checked in full."""
    live = ~r.idle
    o, d = np.where(live[:, None], r.o, 0).astype(np.float64), np.where(live[:, None], r.d, [0, 0, 1]).astype(np.float64)
    _, _, shaky, _ = plane_view(objs, o, d, np.where(live, r.dist, 1))
    bad = shaky.any(1) & live
    if far:
        sph = objs[objs["type"] == abi.RTX_SPHERE]
        _, _, _, _, _, _, _, gdet, _ = RX._sph_part(o, d, tuple(sph[c].astype(np.float64) for c in ("p0", "radius", "epsilon")))
        bad |= ((gdet > GRAZE[0]) & (gdet < GRAZE[1])).any(1) & live
    for i in np.nonzero(bad)[0]:
        pk = np.arange(i - i % 64, min(i - i % 64 + 64, r.n))
        ok = pk[~bad[pk] & live[pk]]
        j = ok[np.abs(ok - i).argmin()]
        for x in (r.o, r.d, r.dist, r.light, r.target_far):
            x[i] = x[j]
    for _ in range(8):
        _, _, _, short = plane_view(objs, np.where(live[:, None], r.o, 0), np.where(live[:, None], r.d, [0, 0, 1]), np.where(live, r.dist, 1))
        m = short.any(1) & live
        if not m.any():
            break
        r.dist[m] *= np.float32(0.97)
    return int(bad.sum())


def families(objs, name, scene):
    """{family: Rays} for a scene's records (fixed seeds).  `name`: the variant; a tiny scene has no
    sponge axes of its own, so its families are the world variant's."""
    rx = RX.families(objs, name if scene != "tiny" else "world")
    rs = np.random.RandomState(20250919 + (name == "rotated") + 2 * SCENES.index(scene))
    lo, hi = RX.bounds(objs)
    diam = float(np.linalg.norm(hi - lo))
    rad = 0.5 * (hi - lo).max()
    out = {"light": _light_family(rs, objs, lo, hi)}
    for fam in FROM_RX:  # dist: beyond the scene, or a uniform fraction of its diameter (some rays end inside a mesh)
        o, d = rx[fam]
        dist = np.where(rs.randint(0, 2, size=len(o)) == 1, 4.0 * diam + np.linalg.norm(o - 0.5 * (lo + hi), axis=1),
                        rs.uniform(0.02, 1.0, size=len(o)) * diam)
        out[fam] = Rays(o, d, dist)
    o, d = _through_family(rs, objs, name if scene != "tiny" else "world")
    out["through"] = Rays(o, d, np.full(len(o), 4.0 * diam))
    o, d = _far_family(rs, lo, hi, rad)
    out["far60"] = Rays(o, d, np.full(len(o), 60.0 * rad + 2.0 * diam))
    replaced = {fam: _settle(objs, out[fam], fam == "far60") for fam in out}
    assert max(replaced.values()) <= N_RAYS // 32, replaced  # (3 % of a family at most: the families stay what they are)
    # idle: the incoherent rays, three of every eight made idle in turn (dist 0, negative, NaN, a NaN
    # direction component), every fourth wave idle altogether
    src = out["incoherent"]
    o, d, dist = src.o.copy(), src.d.copy(), src.dist.copy()
    i = np.arange(len(o))
    how = np.where((i // 64) % 4 == 3, i % 4, np.where(i % 8 < 3, (i // 8) % 4, -1))
    dist[how == 0] = 0.0
    dist[how == 1] = -dist[how == 1]
    dist[how == 2] = np.nan
    d[how == 3, (i[how == 3] // 3) % 3] = np.nan
    out["idle"] = Rays(o, d, dist, None, how >= 0)
    assert set(out) == set(FAMILIES) and all(r.n == N_RAYS for r in out.values())
    for fam, r in out.items():
        live = ~r.idle
        assert np.isfinite(r.dist[live]).all() and (r.dist[live] > 0).all(), fam
    return out


def mixed(fams):
    """every family in one batch under a fixed permutation: (Rays, perm) with batch[i] = concatenation[perm[i]]"""
    cat = lambda k: np.concatenate([getattr(fams[f], k) for f in FAMILIES])
    perm = np.random.RandomState(20250920).permutation(len(FAMILIES) * N_RAYS)
    return Rays(cat("o"), cat("d"), cat("dist"), cat("light"), cat("idle"), cat("target_far")).take(perm), perm


# ---- expected answers ----
class Pairs:
    """a batch's candidate (ray, triangle or sphere) pairs and the float64 view of its (ray, plane) pairs"""


def candidates(objs, rays):
    """the float64 part of the expected answers (no device, no oracle): the candidate pairs of the live
    rays with the spheres' geometric discriminant and entry distance, and the planes decided"""
    live = np.nonzero(~rays.idle)[0]
    ref = RX.reference(objs, rays.o[live], rays.d[live])
    P = Pairs()
    bounded = objs["type"][ref.cand_obj] != abi.RTX_PLANE
    P.pr, P.po = live[ref.cand_ray[bounded]], ref.cand_obj[bounded]
    P.gdet, P.gt = ref.cand_gdet[bounded], ref.cand_gt[bounded]
    P.sphere = objs["type"][P.po] == abi.RTX_SPHERE
    pl, hit, shaky, short = plane_view(objs, rays.o[live], rays.d[live], rays.dist[live])
    shaky = shaky | short
    P.plane_ray, P.plane_obj = live[np.nonzero(hit)[0]], pl[np.nonzero(hit)[1]]
    P.plane_shaky = int(shaky.sum())
    P.plane_pairs = hit.size
    return P


def far_exempt(P, far, hit, dist):
    """the accepted pairs a far ray's walk may leave out (DESIGN §7.3's exception): a far ray's sphere,
    unless float64 geometry vouches for the hit (the ray clearly meets the sphere, well under dist)"""
    opt = far[P.pr] & P.sphere & hit
    vouched = (P.gdet > SPHERE_CLEAR) & (P.gt + 1e-4 + 32 * RX.E24 * np.abs(P.gt) < dist[P.pr]) & (P.gt > 1e-3)
    return opt & ~vouched


def expected(objs, mats, rays, P, hit):
    """(blocked (n,) bool, transmittance (n, 3) float32, exponents (n, 3)) from the pairs' decisions `hit`
    (any_pairs on P.pr, P.po) and the planes; the light object is left out; idle rays are unblocked, 1"""
    n = rays.n
    pr = np.concatenate([P.pr[hit], P.plane_ray])
    po = np.concatenate([P.po[hit], P.plane_obj])
    keep = po != rays.light[pr]
    pr, po = pr[keep], po[keep]
    blocked = np.zeros(n, bool)
    blocked[pr[~mats.transparent[po]]] = True
    expo = np.zeros((n, 3), np.int64)
    tr = mats.transparent[po]
    np.add.at(expo, (pr[tr], mats.channel[po[tr]]), 1)
    assert expo.max() <= MAX_EXPONENT
    tm = np.ldexp(np.float32(1), -expo).astype(np.float32)
    tm[blocked] = 0
    assert not blocked[rays.idle].any() and (tm[rays.idle] == 1).all()
    return blocked, tm, expo


class Data:
    """a batch in a scene: its candidate pairs, their decisions by `kat` (rtxpy.gpu_kat on the device, the
    oracle's on the CPU) and the expected answers"""

    def __init__(self, objs, mats, rays, kat, P=None):
        self.rays = rays
        self.P = P if P is not None else candidates(objs, rays)
        self.hit = RX.any_pairs(kat, objs, rays.o, rays.d, rays.dist, self.P.pr, self.P.po)
        self.blocked, self.tm, self.expo = expected(objs, mats, rays, self.P, self.hit)

    def exempt(self, far):
        return int(far_exempt(self.P, far, self.hit, self.rays.dist.astype(np.float64)).sum())
