"""A catalogue of small scenes whose geometry reaches the branches of the builders, collapses and quantisers
that well-behaved meshes never reach, with ray families and brute-force answers for them (DESIGN §7.6;
test_hard_meshes.py on the CPU, test_gpu_tree_audit.py and test_gpu_hard_meshes.py on the GPU).

  dupes     one triangle, 600 exact copies: equal centroids (the index split), equal Morton codes
  flat      a 24 x 24 grid of quads in a plane z = const: a zero-extent axis, the frame-scale floor
  flat_rot  the same grid under scene6's rotation: the rotated tree frame on a flat mesh
  slivers   500 needles along a diagonal and 50 zero-area triangles (two equal vertices, or collinear)
  scales    an 80-triangle icosphere at scales 2^-k, k = 0..20, a triangle 1000 units long, a sphere of
            radius 500 and one of 1e-4: primitives far below a grid step, large node exponents
  offset    a 320-triangle icosphere of size 1 centred at (1e4, -1e4, 1e4)
  mixed     300 triangles and 40 spheres, a third on transparent materials, an emitter sphere, an emitter
            triangle and two planes: tmask, emitters left out of the 8-wide tree, the sphere flag
  count0 .. count1025   0, 1, 2, 8, 9, 1024 and 1025 small random triangles over a plane: the empty ref, a
            single-leaf root, the boundaries of RTX_WALK_AUTO

The scene loader demands an emitter in every scene, so every JSON ends with a small emitter sphere; except in
`mixed`, whose emitters belong to it, the scene handed to the tests is that scene without its last object
and without emitters (Stripped), so that the meshes stay what the table says.

Brute force: the float32 intersectors (rtx_kat on the device, the oracle's kat on the CPU) on every (ray,
object) pair of a scene.  It does not depend on any tree.
"""
import copy
import json
import os

import numpy as np

import conftest as C
import rays_exhaustive as RX
import shadow_exhaustive as SX
import rtxpy
from rtxpy import abi

COUNTS = (0, 1, 2, 8, 9, 1024, 1025)
MESHES = ("dupes", "flat", "flat_rot", "slivers", "scales", "offset", "mixed")
SCENES = MESHES + tuple("count%d" % n for n in COUNTS)
FAMILIES = ("inbox", "vertex", "graze", "tiny")
N_RAYS = 512
SEGMENT = {"inbox": 1.0, "vertex": 0.5, "graze": 2.0, "tiny": 0.25}  # shadow segment lengths, in box diagonals
MAT_GREY, MAT_A, MAT_B, MAT_C = 2, 3, 4, 5
SCALES_K = 21        # icospheres of `scales`: k = 0 .. 20
SCALES_TRIS = 80
ROTATION = RX.ROTATION["rotated"]  # scene6.json's own


# ---- meshes: float32 (n, 3, 3) ----
def icosphere(level):
    """a unit icosphere: 20 * 4^level triangles"""
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = np.array(v, np.float64)
    t = v[np.array(f)]
    for _ in range(level):
        a, b, c = t[:, 0], t[:, 1], t[:, 2]
        ab, bc, ca = a + b, b + c, c + a
        t = np.concatenate([np.stack(x, 1) for x in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    return t / np.linalg.norm(t, axis=2, keepdims=True)


def _dupes():
    return np.repeat(np.array([[[-1.0, -0.8, 2.0], [1.1, -0.7, 2.6], [0.1, 1.0, 2.2]]], np.float32), 600, 0)


def _flat():
    g = np.linspace(-1.2, 1.2, 25)
    x0, y0 = np.meshgrid(g[:-1], g[:-1], indexing="ij")
    x1, y1 = np.meshgrid(g[1:], g[1:], indexing="ij")
    z = np.full(x0.shape, 2.5)
    q = lambda x, y: np.stack([x, y, z], -1)
    a, b, c, d = q(x0, y0), q(x1, y0), q(x1, y1), q(x0, y1)
    return np.concatenate([np.stack([a, b, c], 2).reshape(-1, 3, 3), np.stack([a, c, d], 2).reshape(-1, 3, 3)]).astype(np.float32)


def _slivers():
    """needles along the diagonal (1, 1, 1) of a 2-unit cube: 0.5 long, 2^-9 wide; the zero-area triangles on
    dyadic coordinates, so that the loader's e1 and e2 are exactly parallel (or zero)"""
    rs = np.random.RandomState(11)
    u = np.array([1.0, 1.0, 1.0]) / 3 ** 0.5
    w = np.array([1.0, -1.0, 0.0]) / 2 ** 0.5
    s = rs.uniform(-1.0, 1.0, size=(500, 1))
    side = rs.normal(size=(500, 3)) * 0.02
    p0 = s * u + side + [0.0, 0.0, 2.5]
    need = np.stack([p0, p0 + 0.5 * u, p0 + 2.0 ** -9 * w], 1)
    g = lambda n: np.round(rs.uniform(-1, 1, size=(n, 3)) * 64) / 64 + [0.0, 0.0, 2.5]
    a, v = g(50), np.round(rs.uniform(-0.25, 0.25, size=(50, 3)) * 64) / 64
    v[(v == 0).all(1)] = 1 / 64
    zero = np.stack([a, a + v, a + 2 * v], 1)  # collinear
    zero[:25, 2] = zero[:25, 1]               # two equal vertices
    zero[:5, 1] = zero[:5, 0]                 # ... all three
    mesh = np.concatenate([need, zero])
    return mesh[rs.permutation(len(mesh))].astype(np.float32)


def _scales():
    ico = icosphere(1)
    assert len(ico) == SCALES_TRIS
    parts = [2.0 ** -k * (0.25 * ico + np.array([1.0, 0.7, 0.3])) for k in range(SCALES_K)]
    long_one = np.array([[[-500.0, -90.0, -300.0], [500.0, -90.0, -300.0], [0.0, -90.0, 600.0]]])
    return np.concatenate(parts + [long_one]).astype(np.float32)


def _offset():
    return (0.5 * icosphere(2) + np.array([1e4, -1e4, 1e4])).astype(np.float32)


def _random_tris(rs, n, size, lo, hi):
    c = rs.uniform(lo, hi, size=(n, 1, 3))
    return (c + rs.uniform(-size, size, size=(n, 3, 3))).astype(np.float32)


# ---- scenes ----
def _materials(tpl):
    m = json.loads(json.dumps(tpl["Materials"]))
    for k, key in ((MAT_A, "A"), (MAT_B, "B"), (MAT_C, "C")):
        g = json.loads(json.dumps(m[MAT_GREY]))
        g["id"], g["kt"] = k, SX.KT[key]
        m.append(g)
    return m


def _mesh(f, m, eps=None, rot=(0.0, 0.0, 0.0), pos=(0.0, 0.0, 0.0)):
    p = {"material": m, "filename": "meshes/" + f, "position": list(pos), "rotation": list(rot), "scale": 1.0}
    if eps is not None:
        p["epsilon"] = eps
    return {"type": "Mesh", "parameters": p}


def _sphere(m, pos, r, **kw):
    return {"type": "Sphere", "parameters": dict({"material": m, "position": list(pos), "radius": r}, **kw)}


def _plane(m, pos, nrm):
    return {"type": "Plane", "parameters": {"material": m, "epsilon": 0.00025, "position": list(pos), "normal": list(nrm)}}


def _objects(name, stl):
    """the scene's objects, the loader's emitter last; stl(file, triangles) writes a mesh"""
    light = lambda pos, r=0.05: [_sphere(1, pos, r, epsilon=0.0003, lights=4)]
    if name == "dupes":
        stl("dupes.stl", _dupes())
        return [_mesh("dupes.stl", 0)] + light([0.0, 0.0, 2.3])
    if name in ("flat", "flat_rot"):
        stl("flat.stl", _flat())
        if name == "flat":
            return [_mesh("flat.stl", 0)] + light([0.0, 0.0, 2.5])
        return [_mesh("flat.stl", 0, rot=ROTATION, pos=[0.3, -0.1, 0.4])] + light([0.0, 0.0, 2.5])
    if name == "slivers":
        stl("slivers.stl", _slivers())
        # (an epsilon of its own: the default, 0.003 area^0.75, is 0 or NaN for a zero-area triangle, and with 0 float32's
        # rounding of the determinant lets the intersector accept hits on collinear vertices)
        return [_mesh("slivers.stl", 0, eps=1e-6)] + light([0.0, 0.0, 2.5])
    if name == "scales":  # (the default epsilon of a triangle, 0.003 area^0.75, would reject every hit of the small ones)
        stl("scales.stl", _scales())
        return [_mesh("scales.stl", 0, eps=1e-30), _sphere(MAT_GREY, [0.0, -600.0, 0.0], 500.0, epsilon=1e-3),
                _sphere(MAT_GREY, [2.0 ** -13, 2.0 ** -12, 2.0 ** -13], 1e-4, epsilon=1e-9)] + light([0.5, 0.5, 0.5])
    if name == "offset":
        stl("offset.stl", _offset())
        return [_mesh("offset.stl", 0)] + light([1e4, -1e4, 1e4])
    if name == "mixed":
        rs = np.random.RandomState(23)
        for f, n in (("mixed_o.stl", 200), ("mixed_a.stl", 50), ("mixed_b.stl", 50)):
            stl(f, _random_tris(rs, n, 0.15, [-1.5, -1.0, 1.5], [1.5, 1.0, 3.5]))
        sph = [_sphere((MAT_GREY, 0, MAT_C)[k % 3], rs.uniform([-1.5, -1.0, 1.5], [1.5, 1.0, 3.5]), float(rs.uniform(0.05, 0.2)))
               for k in range(40)]
        return ([_mesh("mixed_o.stl", 0), _mesh("mixed_a.stl", MAT_A), _mesh("mixed_b.stl", MAT_B)] + sph
                + [_plane(MAT_C, [0.0, -3.0, 0.0], [0.0, 1.0, 0.0]), _plane(MAT_GREY, [0.0, -3.5, 0.0], [0.0, 1.0, 0.0]),
                   {"type": "Triangle", "parameters": {"material": 1, "vertex_1": [-0.9, 0.9, 1.6], "vertex_2": [0.1, 0.9, 1.4],
                                                       "vertex_3": [-0.5, 1.1, 2.6], "lights": 4}}]
                + light([0.4, 0.6, 2.5], 0.2))
    n = int(name[len("count"):])
    objs = []
    if n:
        stl(name + ".stl", _random_tris(np.random.RandomState(100 + n), n, 0.12, [-1.0, -1.0, 1.5], [1.0, 1.0, 3.5]))
        objs.append(_mesh(name + ".stl", 0))
    return objs + [_plane(MAT_GREY, [0.0, -1.5, 0.0], [0.0, 1.0, 0.0])] + light([0.0, 0.0, 2.5])


def write_scenes(tmp):
    """every scene of the catalogue under `tmp`: {name: path of its JSON}"""
    tmp = str(tmp)
    os.makedirs(os.path.join(tmp, "meshes"), exist_ok=True)
    with open(os.path.join(C.SCENES, "scene6.json")) as fh:
        tpl = json.load(fh)
    stl = lambda f, tris: rtxpy.write_stl(os.path.join(tmp, "meshes", f), tris)
    out = {}
    for name in SCENES:
        d = copy.deepcopy(tpl)
        d["Materials"] = _materials(tpl)
        d["Objects"] = _objects(name, stl)
        out[name] = os.path.join(tmp, name + ".json")
        with open(out[name], "w") as fh:
            json.dump(d, fh)
    return out


class Stripped:
    """a loaded scene without its last object (the loader's emitter) and without emitters: the same records,
    a description of its own"""

    def __init__(self, scene):
        self._scene = scene
        d = abi.SceneDesc.from_buffer_copy(scene.desc)
        assert d.num_emitters == 1 and d.emitters[0] == d.num_objects - 1
        d.num_objects -= 1
        d.num_emitters = 0
        d.emitters = None
        self.desc = d

    def close(self):
        self._scene.close()


def load(name, path):
    s = RX.load(path)
    return s if name == "mixed" else Stripped(s)


def emitters_of(scene):
    return [int(scene.desc.emitters[i]) for i in range(scene.desc.num_emitters)]


def transparent_of(scene, objs):
    tr = np.array([scene.desc.materials[i].transparent != 0 for i in range(scene.desc.num_materials)])
    return tr[objs["material"]]


def is_bounded(objs):
    return objs["type"] != abi.RTX_PLANE


def zero_area(objs):
    """triangles whose edges are exactly parallel (or zero)"""
    e1, e2 = objs["e1"].astype(np.float64), objs["e2"].astype(np.float64)
    return (objs["type"] == abi.RTX_TRIANGLE) & (np.cross(e1, e2) == 0).all(1)


def scales_k(objs):
    """per object of `scales`: the k of its icosphere; the long triangle -1, the large sphere -1, the small one 13"""
    k = np.full(len(objs), -1)
    k[:SCALES_K * SCALES_TRIS] = np.arange(SCALES_K * SCALES_TRIS) // SCALES_TRIS
    k[np.nonzero((objs["type"] == abi.RTX_SPHERE) & (objs["radius"] < 1e-3))[0]] = 13
    return k


# ---- ray families ----
def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _box(objs):
    if not is_bounded(objs).any():
        return np.array([-1.0, -1.0, 1.5]), np.array([1.0, 1.0, 3.5])
    return RX.bounds(objs)


def _sizes(objs):
    """per bounded object: the diagonal of its box"""
    lo, hi = np.zeros((len(objs), 3)), np.zeros((len(objs), 3))
    tri, sph = objs["type"] == abi.RTX_TRIANGLE, objs["type"] == abi.RTX_SPHERE
    v = np.stack([objs["p0"], objs["p1"], objs["p2"]]).astype(np.float64)
    lo[tri], hi[tri] = v.min(0)[tri], v.max(0)[tri]
    r = objs["radius"].astype(np.float64)[:, None]
    lo[sph], hi[sph] = (objs["p0"] - r)[sph], (objs["p0"] + r)[sph]
    return np.linalg.norm(hi - lo, axis=1)


# What float32's intersectors cannot resolve, by float64 geometry on the float32 records.  The walks promise
# every hit whose ray meets the primitive's padded box before the closest t so far; the brute force promises
# whatever float32 accepts.  The two part where float32 accepts a geometric miss or returns a t below the
# box's entry, and that takes one of two things (DESIGN §7.6 has a ray of each kind):
#   - a ray that meets a triangle at its border (barycentric margin within rays_exhaustive's ambiguity width)
#     nearly along its plane, eps <= |e1 . (d x e2)| < OBLIQUE eps: 1 / a amplifies float32's rounding of u, v
#     and t by up to |e1| |e2| / eps;
#   - a sphere whose geometric discriminant lies within float32's rounding of b^2 - c, SPHERE_BAND 2^-24 max(|o - c|^2,
#     b^2): from D away that is a sphere of radius below about 2e-3 D, or a graze of a larger one.
OBLIQUE = 16.0
SPHERE_BAND = 64.0


def undecided(objs, o, d, chunk=256):
    """per ray: does it meet a triangle or a sphere in one of the two ways above?"""
    f8 = lambda x: x.astype(np.float64)
    tri, sph = objs[objs["type"] == abi.RTX_TRIANGLE], objs[objs["type"] == abi.RTX_SPHERE]
    out = np.zeros(len(o), bool)
    for i0 in range(0, len(o), chunk):
        oc, dc = f8(o[i0:i0 + chunk]), f8(d[i0:i0 + chunk])
        bad = np.zeros(len(oc), bool)
        if len(tri):
            T = tuple(f8(tri[c]) for c in ("p0", "e1", "e2", "n", "epsilon"))
            with np.errstate(all="ignore"):
                _, t, _, _, _, margin, M, _, _ = RX._tri_part(oc, dc, T)
                a = np.einsum("tk,rtk->rt", T[1], np.cross(dc[:, None, :], T[2][None]))
                eps = T[4][None]
                bad |= ((np.abs(a) >= eps * (1 - 1e-3)) & (np.abs(a) < OBLIQUE * eps) & (np.abs(margin) <= M) & (t > 0)).any(1)
        if len(sph):
            c, r = f8(sph["p0"]), f8(sph["radius"])
            rel = oc[:, None, :] - c[None]
            bg = -(dc[:, None, :] * rel).sum(-1) / np.linalg.norm(dc, axis=1)[:, None]
            rel2 = (rel * rel).sum(-1)
            gdet = bg * bg - (rel2 - (r * r)[None])
            band = SPHERE_BAND * RX.E24 * np.maximum(rel2, bg * bg)
            bad |= ((np.abs(gdet) <= band) & (bg + np.sqrt(np.maximum(gdet, 0)) + np.sqrt(band) > 0)).any(1)
        out[i0:i0 + chunk] = bad
    return out


def _settle(objs, r):
    """the family made decidable: an undecided ray gives way to the nearest decided ray of its 64-ray packet"""
    bad = undecided(objs, r.o, r.d)
    for i in np.nonzero(bad)[0]:
        pk = np.arange(i - i % 64, min(i - i % 64 + 64, r.n))
        ok = pk[~bad[pk]]
        j = ok[np.abs(ok - i).argmin()]
        for x in (r.o, r.d, r.dist):
            x[i] = x[j]
    return int(bad.sum())


def families(objs, name):
    """{family: shadow_exhaustive.Rays} for scene `name`: N_RAYS float32 rays each (fixed seeds) with the
    family's segment length; rays too close to a plane's thresholds give way to a neighbour (SX._settle)"""
    rs = np.random.RandomState(20260131 + SCENES.index(name))
    n = N_RAYS
    lo, hi = _box(objs)
    ce, he = 0.5 * (lo + hi), 0.5 * (hi - lo)
    he = np.maximum(he, 0.1 * he.max())  # (a flat mesh: origins off its plane too)
    ext, diam = float(2 * he.max()), float(np.linalg.norm(2 * he))
    inbox = lambda m=n: rs.uniform(ce - 1.2 * he, ce + 1.2 * he, size=(m, 3))
    dirs = lambda m=n: _unit(rs.normal(size=(m, 3)))
    bounded = np.nonzero(is_bounded(objs))[0]
    tri = objs[(objs["type"] == abi.RTX_TRIANGLE) & np.isfinite(objs["n"]).all(1)]
    out = {"inbox": (inbox(), dirs())}
    if not len(bounded):
        out["vertex"], out["graze"], out["tiny"] = (inbox(), dirs()), (inbox(), dirs()), (inbox(), dirs())
    else:
        anytri = objs[objs["type"] == abi.RTX_TRIANGLE]
        # vertex: exactly at vertices and edge midpoints, from 2 to 20 sizes of the triangle away (half an extent at most)
        t = anytri[rs.randint(0, len(anytri), size=n)]
        vs = np.stack([t["p0"], t["p1"], t["p2"]], 1).astype(np.float64)
        k = rs.randint(0, 3, size=n)
        a, b = vs[np.arange(n), k], vs[np.arange(n), (k + 1) % 3]
        target = np.where((rs.randint(0, 2, size=n) == 1)[:, None], a, 0.5 * (a + b))
        tsize = np.maximum(np.linalg.norm(vs.max(1) - vs.min(1), axis=1), 1e-9 * ext)[:, None]
        away = np.minimum(tsize * rs.uniform(2, 20, size=(n, 1)), rs.uniform(0.1, 0.5, size=(n, 1)) * ext)
        w = dirs()  # not along the triangle's own plane (undecided() below; its neighbours' planes are left to it)
        nn = np.where(np.isfinite(t["n"]).all(1)[:, None], t["n"], 0).astype(np.float64)
        c = (w * nn).sum(1, keepdims=True)
        w = np.where(np.abs(c) < 0.25, _unit(w + np.where(c < 0, -0.5, 0.5) * nn), w)
        o = (target - w * away).astype(np.float32).astype(np.float64)
        out["vertex"] = (o, _unit(target - o))
        # graze: from within 1e-3 extents (64e-3 sizes of the triangle at most) of a triangle's plane, nearly along it
        t = tri[rs.randint(0, len(tri), size=n)]
        u, v = rs.uniform(size=n), rs.uniform(size=n)
        fold = u + v > 1
        u[fold], v[fold] = 1 - u[fold], 1 - v[fold]
        nn = t["n"].astype(np.float64)
        p = t["p0"] + u[:, None] * t["e1"].astype(np.float64) + v[:, None] * t["e2"].astype(np.float64)
        w = dirs()
        w = _unit(w - (w * nn).sum(1, keepdims=True) * nn)  # in the plane
        tilt = rs.uniform(-1e-2, 1e-2, size=(n, 1))
        d = _unit(w + tilt * nn)
        vs = np.stack([t["p0"], t["p1"], t["p2"]], 1).astype(np.float64)
        tsize = np.maximum(np.linalg.norm(vs.max(1) - vs.min(1), axis=1), 1e-9 * ext)[:, None]
        back = np.minimum(tsize * rs.uniform(1, 10, size=(n, 1)), rs.uniform(0.05, 0.5, size=(n, 1)) * ext)
        o = p - w * back + nn * rs.uniform(-1e-3, 1e-3, size=(n, 1)) * np.minimum(ext, 64 * tsize)
        if name == "flat":  # a quarter exactly in the plane's direction, the zero signed both ways
            d[::4, 2] = np.where(rs.randint(0, 2, size=len(d[::4])) == 1, -0.0, 0.0)
            d[::4] = _unit(d[::4])
        out["graze"] = (o, d)
        # tiny: at the centroids of the smallest tenth, from 4 to 16 of their sizes away (half an extent at most)
        size = _sizes(objs)[bounded]
        small = bounded[np.argsort(size, kind="stable")[:max(1, len(bounded) // 10)]]
        pick = small[rs.randint(0, len(small), size=n)]
        t = objs[pick]
        istri = (t["type"] == abi.RTX_TRIANGLE)[:, None]
        target = np.where(istri, (t["p0"].astype(np.float64) + t["p1"] + t["p2"]) / 3, t["p0"].astype(np.float64))
        away = np.maximum(_sizes(objs)[pick], 1e-6 * ext)[:, None] * rs.uniform(4, 16, size=(n, 1))
        away = np.minimum(away, rs.uniform(0.1, 0.5, size=(n, 1)) * ext)  # (large primitives: within the scene)
        o = (target - dirs() * away).astype(np.float32).astype(np.float64)
        out["tiny"] = (o, _unit(target - o))
    res = {}
    for fam in FAMILIES:
        o, d = out[fam]
        r = SX.Rays(o, d, np.full(n, SEGMENT[fam] * diam))
        assert np.isfinite(r.o).all() and np.abs(np.linalg.norm(r.d.astype(np.float64), axis=1) - 1).max() < 1e-6
        r.replaced = _settle(objs, r) + SX._settle(objs, r, False)
        assert r.replaced <= n // 32, (name, fam, r.replaced)  # (3 % of a family at most: the families stay what they are)
        res[fam] = r
    if name == "flat":
        z = res["graze"].d[:, 2]
        assert (z == 0).sum() >= n // 8 and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    return res


def batch(fams):
    """the families in one batch: shadow_exhaustive.Rays of len(FAMILIES) * N_RAYS rays, and each family's rows"""
    cat = lambda k: np.concatenate([getattr(fams[f], k) for f in FAMILIES])
    return SX.Rays(cat("o"), cat("d"), cat("dist")), {f: slice(i * N_RAYS, (i + 1) * N_RAYS) for i, f in enumerate(FAMILIES)}


def assert_near(scene, objs, o, frame_world=False):
    """no origin is far (rtx_math.h tf_far): all lie within 3 radii of the bounded objects' centre"""
    if not is_bounded(objs).any():
        return
    rotated, R, c, _ = rtxpy.tree_frame(scene)
    lo, hi = RX.bounds(objs)
    o = o.astype(np.float64)
    if rotated and not frame_world:
        ce = c.astype(np.float64)
        dist = np.abs((o - ce) @ R.astype(np.float64).T).max(1)
    else:
        ce = 0.5 * lo + 0.5 * hi
        dist = np.abs(o - ce).max(1)
    rad = max(np.abs(lo - ce).max(), np.abs(hi - ce).max())
    assert (dist <= 3.0 * rad).all(), float((dist / rad).max())
    assert not RX.far_mask(scene, objs, o.astype(np.float32), frame_world=frame_world).any()


# ---- brute force ----
class Brute:
    """every (ray, object) pair of a batch decided by `kat`'s float32 intersectors:
      t          the least accepted t per ray, float32, 0 where nothing is hit
      pr, po, pt the accepted closest-hit pairs (ray, object, t), sorted by ray
      blocked, tm, expo   shadow_exhaustive.expected over all pairs for the batch's segments"""

    def __init__(self, kat, scene, objs, rays, chunk=128):
        n, m = rays.n, len(objs)
        self.n_objs = m
        every = np.arange(m)
        bounded = np.nonzero(is_bounded(objs))[0]
        tmin = np.zeros(n, np.float32)
        acc, shadow = [], []
        for i0 in range(0, n, chunk):
            rows = np.arange(i0, min(i0 + chunk, n))
            pr, po = np.repeat(rows, m), np.tile(every, len(rows))
            hit, t = RX.kat_pairs(kat, objs, rays.o, rays.d, pr, po)
            tm = np.full(n, np.inf, np.float32)
            np.minimum.at(tm, pr[hit], t[hit])
            tmin[rows] = np.where(np.isinf(tm[rows]), 0, tm[rows])
            acc.append((pr[hit], po[hit], t[hit]))
            if len(bounded):
                pr, po = np.repeat(rows, len(bounded)), np.tile(bounded, len(rows))
                sh = RX.any_pairs(kat, objs, rays.o, rays.d, rays.dist, pr, po)
                shadow.append((pr[sh], po[sh]))
        self.t = tmin
        self.pr, self.po, self.pt = (np.concatenate(x) for x in zip(*acc))
        P = SX.Pairs()
        P.pr, P.po = (np.concatenate(x) for x in zip(*shadow)) if shadow else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        pl, phit, shaky, short = SX.plane_view(objs, rays.o, rays.d, rays.dist)
        assert not shaky.any() and not short.any()  # (families() settled them)
        P.plane_ray, P.plane_obj = np.nonzero(phit)[0], pl[np.nonzero(phit)[1]]
        self.P = P
        mats = SX.Mats(scene, objs)
        self.blocked, self.tm, self.expo = SX.expected(objs, mats, rays, P, np.ones(len(P.pr), bool))

    def attains(self, rays, objects, tbits):
        """is (rays[i], objects[i]) an accepted pair whose t has the bits tbits[i]?"""
        return RX.attains(self.n_objs, self.pr, self.po, np.ones(len(self.pr), bool), self.pt, rays, objects, tbits)

    def accepted_below(self, tmax):
        """per ray: is some pair accepted with t < tmax[ray]?"""
        out = np.zeros(len(self.t), bool)
        out[self.pr[self.pt < np.asarray(tmax, np.float32)[self.pr]]] = True
        return out

    def closest_objects(self):
        """per ray: an object attaining t (-1 on a miss)"""
        obj = np.full(len(self.t), -1)
        at = self.pt.view(np.uint32) == self.t.view(np.uint32)[self.pr]
        obj[self.pr[at][::-1]] = self.po[at][::-1]
        return obj
