"""Ray queries against a brute-force minimum (DESIGN §7.3 "Exhaustive check").

For a few thousand incoherent and degenerate rays (rays_exhaustive.py: origins all over the scene and
a hair above its surfaces, directions with exact zero components, rays at vertices and edges, rays
in the sponge's grid planes, rays from 60 and 2000 radii, and all of them mixed in one batch) the
closest query's t must equal, bit for bit, the minimum over the ray's candidate objects of the
device's own exact intersectors (rtx_kat): whatever the walk, the builder, the leaf size, the trees'
frame, the batch, the order or the flags.  The intersectors themselves are held to the oracle's
(bit for bit) and to a float64 restatement (on the rays where float64 can decide).

One documented exception (rtx_math.h far_sphere_box): a ray whose origin is far
(tf_far) tests a sphere only where its segment up to the closest t so far meets the sphere's padded
world box, because hit_sphere's discriminant cancels from far off and rtx_kat then reports hits of
rays that pass the sphere by.  A far ray's rtx_kat sphere hit is therefore optional (the query's t is
the minimum over the other candidates, or that sphere's own rtx_kat t below it) unless float64 says
the box test must pass: the ray clearly meets the sphere (geometric discriminant above SPHERE_CLEAR r^2) and the
sphere's float64 t lies below every other candidate's rtx_kat t and below tmax.  Such a pair is
mandatory like any other, so a dropped sphere or a box padded too little fails from 2000 radii too.
"""
import numpy as np
import pytest

import rays_exhaustive as RX
import rtxpy
from rtxpy import abi, oracle
from test_gpu_build import GPU_BUILDERS, IDS as BUILDER_IDS

pytestmark = pytest.mark.gpu

U32 = np.uint32
BASE = ("world-auto", "world-bvh2", "rotated-auto", "rotated-bvh2")
CONFIGS = {"world-auto": dict(scene="world", walk=abi.RTX_WALK_AUTO),
           "world-bvh2": dict(scene="world", walk=abi.RTX_WALK_BVH2),
           "rotated-auto": dict(scene="rotated", walk=abi.RTX_WALK_AUTO),
           "rotated-bvh2": dict(scene="rotated", walk=abi.RTX_WALK_BVH2),
           "world-auto-leaf4": dict(scene="world", walk=abi.RTX_WALK_AUTO, leaf=4),
           "world-bvh2-leaf4": dict(scene="world", walk=abi.RTX_WALK_BVH2, leaf=4),
           "rotated-auto-frameworld": dict(scene="rotated", walk=abi.RTX_WALK_AUTO, frame=abi.RTX_FRAME_WORLD)}
CONFIGS.update({"world-auto-" + i: dict(scene="world", walk=abi.RTX_WALK_AUTO, builder=b) for b, i in zip(GPU_BUILDERS, BUILDER_IDS)})
SPHERE_CLEAR = 1e-3  # (a ray this far inside the silhouette passes within 0.9995 r of the centre: inside any box of the sphere)
CLOSEST_FAMILIES = tuple(f for f in RX.FAMILIES if f != "onplane")


class Data:
    """a family's rays in a scene, their float64 reference and rtx_kat on every candidate pair"""

    def __init__(self, objs, o, d):
        self.o, self.d, self.n = o, d, len(o)
        self.ref = RX.reference(objs, o, d)
        self.pr, self.po = self.ref.cand_ray, self.ref.cand_obj
        self.hit, self.t = RX.kat_pairs(rtxpy.gpu_kat, objs, o, d, self.pr, self.po)
        self.objs_type = objs["type"]
        self.sphere = self.objs_type[self.po] == abi.RTX_SPHERE
        self.tmin = RX.ray_min(self.n, self.pr, self.hit, self.t)

    def optional(self, far, live, tmax=None, front=True):
        """the pairs among `live` (accepted by rtx_kat, under tmax) that a query may leave out: a far
        ray's sphere, unless its box test must pass (module docstring).  front: the sphere must also lie
        before every other live candidate (a closest query tests boxes against the closest t so far)."""
        opt = far[self.pr] & self.sphere
        for i in np.nonzero(opt & live & (self.ref.cand_gdet > SPHERE_CLEAR))[0]:
            limit = np.inf if tmax is None else float(tmax[self.pr[i]])
            if front:
                others = live & (self.pr == self.pr[i])
                others[i] = False
                limit = min(limit, float(self.t[others].min())) if others.any() else limit
            t64 = self.ref.cand_gt[i]
            opt[i] = not (t64 + 1e-4 + 32 * RX.E24 * t64 < limit)  # (the other t are float32 values of about t64's size)
        return opt


class Gpu:
    def __init__(self, tmp):
        self.paths = RX.write_scenes(tmp)
        self.scenes, self.objs, self.fams, self.mix, self.data, self.ctx, self.hits = {}, {}, {}, {}, {}, {}, {}

    def scene(self, name):
        if name not in self.scenes:
            self.scenes[name] = RX.load(self.paths[name])
            self.objs[name] = RX.objects_of(self.scenes[name])
            self.fams[name] = RX.families(self.objs[name], name)
            self.mix[name] = RX.mixed(self.fams[name])
        return self.scenes[name]

    def get(self, name, fam):
        if (name, fam) not in self.data:
            self.scene(name)
            self.data[name, fam] = Data(self.objs[name], *self.fams[name][fam])
        return self.data[name, fam]

    def renderer(self, cfg):
        if cfg not in self.ctx:
            c = CONFIGS[cfg]
            r = rtxpy.Renderer(0)
            if "builder" in c:
                r.set_builder(c["builder"])
            r.set_option(abi.RTX_OPT_TRACE_WALK, c["walk"])
            if "leaf" in c:
                r.set_option(abi.RTX_OPT_BVH_LEAF, c["leaf"])
            if "frame" in c:
                r.set_option(abi.RTX_OPT_TREE_FRAME, c["frame"])
            r.upload(self.scene(c["scene"]))
            self.ctx[cfg] = r
        return self.ctx[cfg]

    def far(self, cfg, o):
        name = CONFIGS[cfg]["scene"]
        return RX.far_mask(self.scene(name), self.objs[name], o, frame_world=CONFIGS[cfg].get("frame") == abi.RTX_FRAME_WORLD)

    def closest(self, cfg, fam):
        """the unbounded closest query of a family, traced on its own"""
        if (cfg, fam) not in self.hits:
            D = self.get(CONFIGS[cfg]["scene"], fam)
            self.hits[cfg, fam] = self.renderer(cfg).trace_rays(D.o, D.d)
        return self.hits[cfg, fam]

    def close(self):
        for r in self.ctx.values():
            r.close()
        for s in self.scenes.values():
            s.close()


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    g = Gpu(tmp_path_factory.mktemp("rays_exhaustive_gpu"))
    yield g
    g.close()


def attains(D, n_objs, rays, objects, tbits):
    return RX.attains(n_objs, D.pr, D.po, D.hit, D.t, rays, objects, tbits)


def check_closest(D, n_objs, far, got, tmax=None):
    """got (a query's result dict) against the minimum over D's candidate pairs with t < tmax: t bit for
    bit, object one of those that attain it.  Returns the number of far rays whose t is not that minimum
    because a sphere's rtx_kat hit was culled by its box (module docstring)."""
    live = D.hit if tmax is None else D.hit & (D.t < tmax[D.pr])
    opt = D.optional(far, live, tmax)
    want_all, want = RX.ray_min(D.n, D.pr, live, D.t), RX.ray_min(D.n, D.pr, live & ~opt, D.t)
    t, obj = got["t"], got["object"]
    rest = np.nonzero(t.view(U32) != want_all.view(U32))[0]
    # far rays only: every optional sphere culled, or one of them taken under the strict <
    dropped = far[rest] & (t[rest].view(U32) == want[rest].view(U32))
    taken = attains(D, n_objs, rest, obj[rest], t[rest].view(U32)) & far[rest] & (D.objs_type[obj[rest]] == abi.RTX_SPHERE)
    taken &= (want[rest] == 0) | (t[rest] < want[rest])
    ok = dropped | taken
    assert ok.all(), (int((~ok).sum()), rest[~ok][:8], t[rest][~ok][:8], want_all[rest][~ok][:8], obj[rest][~ok][:8])
    h = np.nonzero(t > 0)[0]
    assert ((t > 0) == (obj >= 0)).all()
    assert attains(D, n_objs, h, obj[h], t[h].view(U32)).all()
    if tmax is not None:
        assert (t[h] < tmax[h]).all()
    return len(rest)


def data_for(gpu, cfg, fam):
    name = CONFIGS[cfg]["scene"]
    D = gpu.get(name, fam)
    return D, len(gpu.objs[name]), gpu.far(cfg, D.o)


# ---- 1. exhaustive closest hit, zero tolerance ----
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_closest_equals_the_minimum_over_the_candidates(gpu, cfg):
    c = CONFIGS[cfg]
    r = gpu.renderer(cfg)
    for fam in CLOSEST_FAMILIES:  # (a context that has not rendered yet: the overflow stack is the query's own)
        D, n_objs, far = data_for(gpu, cfg, fam)
        assert far.all() if fam.startswith("far") else not far.any()
        exempt = check_closest(D, n_objs, far, gpu.closest(cfg, fam))
        held = int((far[D.pr] & D.sphere & D.hit & ~D.optional(far, D.hit)).sum())
        print(cfg, fam, "hits", int((gpu.closest(cfg, fam)["t"] > 0).sum()), "far rays whose sphere hit the box culled", exempt,
              "far sphere hits held to rtx_kat", held)
        assert held >= 5 or not far.any()
        assert exempt == 0 or fam == "far2000"  # (from 60 radii hit_sphere still agrees with the sphere's box)
    scene = gpu.scene(c["scene"])
    r.render(scene.frame(16, 16), rtxpy.default_params())  # fills stats().trace_walk
    st = r.stats()
    assert st.trace_walk == (abi.RTX_WALK_BVH2 if c["walk"] == abi.RTX_WALK_BVH2 else abi.RTX_WALK_W8)
    assert st.tree_rotated == (1 if c["scene"] == "rotated" and "frame" not in c else 0)
    if cfg == "world-bvh2":
        assert st.bvh_depth + 1 > 9  # RTX_TRACE_LSTK: the deeper lane-stack entries live in HBM


# ---- 2. rays in the sponge's grid planes ----
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_onplane_misses_only_edges(gpu, cfg):
    D, n_objs, far = data_for(gpu, cfg, "onplane")
    assert not far.any()
    got = gpu.closest(cfg, "onplane")
    t, obj = got["t"], got["object"]
    h = np.nonzero(t > 0)[0]
    assert ((t > 0) == (obj >= 0)).all()
    assert attains(D, n_objs, h, obj[h], t[h].view(U32)).all()  # the reported object's own rtx_kat t
    assert (D.tmin[h] > 0).all() and (t[h] >= D.tmin[h]).all()  # never below the exhaustive minimum
    differs = t.view(U32) != D.tmin.view(U32)
    # every accepted hit the query passed over lies on a triangle's edge by the float64 reference
    tq = np.where(t > 0, t, np.float32(np.inf))
    passed = D.hit & (D.t < tq[D.pr])
    assert set(np.unique(D.pr[passed])) == set(np.nonzero(differs)[0])
    on_edge = np.abs(D.ref.cand_margin[passed]) <= D.ref.cand_M[passed]  # (NaN for a sphere or a plane: not an edge)
    print(cfg, "onplane: t differs from the exhaustive minimum on", int(differs.sum()), "of", D.n, "rays;",
          int(passed.sum()), "hits passed over,", int((~on_edge).sum()), "of them interior")
    assert on_edge.all()


# ---- 3. batch independence ----
@pytest.mark.parametrize("cfg", BASE)
def test_mixed_batch_returns_the_same_bits(gpu, cfg):
    name = CONFIGS[cfg]["scene"]
    r = gpu.renderer(cfg)
    o, d, perm, _ = gpu.mix[name]
    want = {k: np.concatenate([gpu.closest(cfg, f)[k] for f in RX.FAMILIES])[perm] for k in ("t", "object")}
    fam_of = np.repeat(np.arange(len(RX.FAMILIES)), RX.N_RAYS)[perm]
    row_of = np.tile(np.arange(RX.N_RAYS), len(RX.FAMILIES))[perm]
    n_objs = len(gpu.objs[name])

    def check(got, what):
        assert np.array_equal(got["t"].view(U32), want["t"].view(U32)), (what, int((got["t"] != want["t"]).sum()))
        diff = np.nonzero(got["object"] != want["object"])[0]
        print(cfg, what, "object differs on", len(diff), "of", len(o))
        for k, f in enumerate(RX.FAMILIES):  # only exact ties: both objects' own rtx_kat t are the reported bits
            i = diff[fam_of[diff] == k]
            D = gpu.get(name, f)
            for ob in (got["object"][i], want["object"][i]):
                assert attains(D, n_objs, row_of[i], ob, got["t"][i].view(U32)).all(), (what, f)

    check(r.trace_rays(o, d), "flags 0")
    check(r.trace_rays(o, d, reorder=True), "reorder")
    try:
        for queues, grab in ((1, 1), (8, 64)):
            r.set_option(abi.RTX_OPT_RAYS_QUEUES, queues)
            r.set_option(abi.RTX_OPT_RAYS_GRAB, grab)
            check(r.trace_rays(o, d), "queues %d grab %d" % (queues, grab))
    finally:
        r.set_option(abi.RTX_OPT_RAYS_QUEUES, 0)
        r.set_option(abi.RTX_OPT_RAYS_GRAB, 0)
    check(r.trace_rays(o, d, count=True), "count")
    far = gpu.far(cfg, o)
    rs = r.ray_stats()
    assert far.sum() >= 2 * RX.N_RAYS
    # (a ray that hits a plane's lower t still walks: only any-hit rays end at a plane)
    assert rs.rays == len(o) and rs.hits == np.count_nonzero(want["t"]) and rs.far_rays == far.sum(), (rs.far_rays, far.sum())


# ---- 4. any hit, exact ----
@pytest.mark.parametrize("cfg", BASE)
def test_any_hit_is_exact(gpu, cfg):
    r = gpu.renderer(cfg)
    rs = np.random.RandomState(11)
    for fam in CLOSEST_FAMILIES:
        D, n_objs, far = data_for(gpu, cfg, fam)
        hit = D.tmin > 0
        tmax = np.where(hit, D.tmin * rs.uniform(0.2, 3.0, D.n), rs.uniform(0.1, 50.0, D.n)).astype(np.float32)
        under = D.hit & (D.t < tmax[D.pr])
        opt = D.optional(far, under, tmax, front=False)  # (an any-hit ray tests every box against tmax itself)
        must = np.zeros(D.n, bool)
        must[D.pr[under & ~opt]] = True
        may = np.zeros(D.n, bool)
        may[D.pr[under]] = True
        assert must.any() and not may.all()
        for reorder in (False, True):
            got = r.trace_rays(D.o, D.d, tmax=tmax, any_hit=True, reorder=reorder)
            t, obj = got["t"], got["object"]
            h = t > 0
            assert np.array_equal(h, obj >= 0)
            assert not (must & ~h).any() and not (h & ~may).any(), (fam, reorder, int((must & ~h).sum()), int((h & ~may).sum()))
            assert far.all() or np.array_equal(h, must)
            i = np.nonzero(h)[0]
            assert attains(D, n_objs, i, obj[i], t[i].view(U32)).all() and (t[i] < tmax[i]).all()
        print(cfg, fam, "any hit", int(must.sum()), "of", D.n, "optional", int((may & ~must).sum()))


# ---- 5. tmax edges ----
@pytest.mark.parametrize("cfg", BASE)
def test_tmax_edges(gpu, cfg):
    r = gpu.renderer(cfg)
    for fam in ("incoherent", "surface"):
        D, n_objs, far = data_for(gpu, cfg, fam)
        full = gpu.closest(cfg, fam)
        assert np.array_equal(full["t"].view(U32), D.tmin.view(U32))
        hit = D.tmin > 0
        inf = np.float32(np.inf)
        above = r.trace_rays(D.o, D.d, tmax=np.where(hit, np.nextafter(D.tmin, inf), inf))
        assert all(np.array_equal(above[k], full[k]) for k in full)
        at = np.where(hit, D.tmin, inf).astype(np.float32)
        exact = r.trace_rays(D.o, D.d, tmax=at)  # strictly below: the closest hit itself is out
        check_closest(D, n_objs, far, exact, tmax=at)
        assert (exact["t"] == 0).all()  # (nothing lies strictly below a minimum)
        print(cfg, fam, "tmax = t: hits left", int((exact["t"] > 0).sum()), "of", int(hit.sum()))
        for tmax in (0.0, -1.0, -np.inf):
            none = r.trace_rays(D.o, D.d, tmax=tmax)
            assert (none["t"] == 0).all() and (none["object"] == -1).all() and (none["material"] == -1).all(), tmax
            anyh = r.trace_rays(D.o, D.d, tmax=tmax, any_hit=True)
            assert (anyh["t"] == 0).all() and (anyh["object"] == -1).all(), tmax
        nan = r.trace_rays(D.o, D.d, tmax=np.nan)  # include/rtx.h: INFINITY (or NaN) = unbounded
        assert all(np.array_equal(nan[k], full[k]) for k in full)


# ---- 6. the device intersectors on the scenes' records ----
@pytest.mark.parametrize("name", ("world", "rotated"))
def test_device_intersectors_equal_the_oracle_on_real_records(gpu, name):
    pairs = wrong = 0
    for fam in RX.FAMILIES:
        D = gpu.get(name, fam)
        hit, t = RX.kat_pairs(oracle.kat, gpu.objs[name], D.o, D.d, D.pr, D.po)
        bad = (hit != D.hit) | (hit & D.hit & (t.view(U32) != D.t.view(U32)))
        pairs += len(bad)
        wrong += int(bad.sum())
        if bad.any():
            print(name, fam, "differs on", int(bad.sum()), "pairs; types", np.unique(gpu.objs[name]["type"][D.po[bad]]))
    print(name, "rtx_kat against the oracle:", wrong, "of", pairs, "candidate pairs differ")
    assert wrong <= 1e-3 * pairs


# ---- 7. float64 on the decisive rays ----
@pytest.mark.parametrize("cfg", BASE)
def test_queries_against_float64_on_decisive_rays(gpu, cfg):
    name = CONFIGS[cfg]["scene"]
    for fam in RX.FLOORED:
        D = gpu.get(name, fam)
        got = gpu.closest(cfg, fam)
        hm, om, rel = RX.compare_with_float64(len(gpu.objs[name]), D.ref, D.pr, D.po, D.hit, D.t, got["t"], got["object"])
        print(cfg, fam, "decisive", int(D.ref.decisive.sum()), "hit/miss differs", hm, "object differs", om, "max rel", rel)
        assert hm == 0 and om == 0 and rel <= RX.T64_BOUND[RX.t64_class(fam)]
