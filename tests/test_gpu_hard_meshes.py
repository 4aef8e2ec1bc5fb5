"""Ray and shadow queries on the hard meshes (hard_meshes.py) against brute force, bit for bit.

Per scene the device's own float32 intersectors (rtx_kat) decide every (ray, object) pair once; that does not
depend on any tree.  Then every builder, both tree frames and both walks must return exactly that: the
closest t's bits with an object that attains them, any-hit answers that are accepted pairs, and the shadow
query's blocked flag and transmittance (powers of two, exact in any order).  No tolerance.

The ray families hold no ray that float32's intersectors cannot decide (hard_meshes.undecided, by float64
geometry alone: test_hard_meshes.py asserts it and counts the rays replaced); DESIGN §7.6 has the three rays
that showed why."""
import numpy as np
import pytest

import hard_meshes as HM
import rays_exhaustive as RX
import rtxpy
from rtxpy import abi

pytestmark = pytest.mark.gpu

U32 = np.uint32
BUILDERS = {"sahhost": abi.RTX_BUILD_SAH_HOST, "sahgpu": abi.RTX_BUILD_SAH_GPU, "lbvh": abi.RTX_BUILD_LBVH_GPU,
            "ploc": abi.RTX_BUILD_PLOC_GPU}
FRAMES = {"auto": abi.RTX_FRAME_AUTO, "world": abi.RTX_FRAME_WORLD}
LINEAR_MAX = 64  # RTX_WALK_LINEAR is asked for on scenes of at most this many bounded objects


class Gpu:
    def __init__(self, tmp):
        self.paths = HM.write_scenes(tmp)
        self.res = {}

    def get(self, name):
        """(scene, records, batch, rows of each family, brute force by rtx_kat)"""
        if name not in self.res:
            scene = HM.load(name, self.paths[name])
            objs = RX.objects_of(scene)
            rays, rows = HM.batch(HM.families(objs, name))
            for world in (False, True):
                HM.assert_near(scene, objs, rays.o, frame_world=world)
            self.res[name] = (scene, objs, rays, rows, HM.Brute(rtxpy.gpu_kat, scene, objs, rays))
        return self.res[name]

    def close(self):
        for s in self.res.values():
            s[0].close()


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    g = Gpu(tmp_path_factory.mktemp("hard_meshes_gpu"))
    yield g
    g.close()


@pytest.fixture(scope="module")
def renderer():
    r = rtxpy.Renderer(0)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def _defaults(renderer):
    yield
    renderer.set_builder(abi.RTX_BUILD_SAH_GPU)
    renderer.set_option(abi.RTX_OPT_SHADOW_WALK, abi.RTX_WALK_AUTO)
    renderer.set_option(abi.RTX_OPT_TRACE_WALK, abi.RTX_WALK_AUTO)
    renderer.set_option(abi.RTX_OPT_BVH_LEAF, 1)
    renderer.set_option(abi.RTX_OPT_SHADOW_LDS_STACK, 8)
    renderer.set_option(abi.RTX_OPT_TREE_FRAME, abi.RTX_FRAME_AUTO)


def rows_of(wrong, rows):
    return {f: int(np.count_nonzero((wrong >= s.start) & (wrong < s.stop))) for f, s in rows.items()}


def check_closest(B, rays, rows, got, what):
    bad = np.nonzero(got["t"].view(U32) != B.t.view(U32))[0]
    assert not len(bad), (what, "closest t differs on", len(bad), rows_of(bad, rows), bad[:6], got["t"][bad[:6]], B.t[bad[:6]])
    hit = np.nonzero(B.t > 0)[0]
    assert (got["object"][B.t == 0] == -1).all(), what
    ok = B.attains(hit, got["object"][hit], got["t"][hit].view(U32))
    assert ok.all(), (what, "object does not attain t on", int((~ok).sum()), hit[~ok][:6])


def check_any(B, rays, rows, got, what):
    want = B.accepted_below(rays.dist)
    bad = np.nonzero((got["t"] != 0) != want)[0]
    assert not len(bad), (what, "any-hit differs on", len(bad), rows_of(bad, rows), bad[:6])
    hit = np.nonzero(want)[0]
    assert (got["t"][hit] < rays.dist[hit]).all(), what
    ok = B.attains(hit, got["object"][hit], got["t"][hit].view(U32))
    assert ok.all(), (what, "any-hit answer is no accepted pair on", int((~ok).sum()), hit[~ok][:6])


def check_shadow(B, rows, got, what):
    bad = np.nonzero(got["blocked"] != B.blocked)[0]
    assert not len(bad), (what, "blocked differs on", len(bad), rows_of(bad, rows), bad[:6], B.blocked[bad[:6]])
    bad = np.nonzero((got["transmittance"].view(U32) != B.tm.view(U32)).any(1))[0]
    assert not len(bad), (what, "transmittance differs on", len(bad), rows_of(bad, rows), bad[:6], got["transmittance"][bad[:6]],
                          B.tm[bad[:6]])


@pytest.mark.parametrize("name", HM.SCENES)
def test_queries_equal_brute_force(gpu, renderer, name):
    scene, objs, rays, rows, B = gpu.get(name)
    r = renderer
    nb = int(HM.is_bounded(objs).sum())
    walks = [("w8", abi.RTX_WALK_W8), ("bvh2", abi.RTX_WALK_BVH2)] + ([("linear", abi.RTX_WALK_LINEAR)] if 0 < nb <= LINEAR_MAX else [])
    seen_t, seen_b = {}, {}
    for builder in BUILDERS:
        for frame in FRAMES:
            r.set_builder(BUILDERS[builder])
            r.set_option(abi.RTX_OPT_TREE_FRAME, FRAMES[frame])
            for wname, walk in walks:
                r.set_option(abi.RTX_OPT_SHADOW_WALK, walk)
                r.set_option(abi.RTX_OPT_SHADOW_LDS_STACK, 8)
                r.upload(scene)
                st = r.stats()
                if nb:
                    assert st.shadow_walk == walk, (name, builder, frame, wname, st.shadow_walk)
                # closest and any hits: the 8-wide tree where this upload built one, and the float BVH2
                for tname, twalk in (("w8", abi.RTX_WALK_W8), ("bvh2", abi.RTX_WALK_BVH2)):
                    if twalk == abi.RTX_WALK_W8 and not st.wide_nodes:
                        continue
                    what = (name, builder, frame, "shadow " + wname, "trace " + tname)
                    r.set_option(abi.RTX_OPT_TRACE_WALK, twalk)
                    got = r.trace_rays(rays.o, rays.d)
                    check_closest(B, rays, rows, got, what)
                    seen_t[what] = got["t"]
                    check_any(B, rays, rows, r.trace_rays(rays.o, rays.d, tmax=rays.dist, any_hit=True), what)
                what = (name, builder, frame, "shadow " + wname)
                got = r.shadow_rays(rays.o, rays.d, rays.dist, -1)
                check_shadow(B, rows, got, what)
                seen_b[what] = got["blocked"]
                if name == "scales" and walk == abi.RTX_WALK_W8:  # the lane stack's spill to HBM on a deep tree
                    r.set_option(abi.RTX_OPT_SHADOW_LDS_STACK, 1)
                    check_shadow(B, rows, r.shadow_rays(rays.o, rays.d, rays.dist, -1), what + ("lds stack 1",))
                    check_shadow(B, rows, r.shadow_rays(rays.o, rays.d, rays.dist, -1, slots=True), what + ("lds stack 1", "slots"))
    # the same bits from every builder, frame and walk (it follows from the above; a failure here names the pair)
    first = next(iter(seen_t))
    for what, t in seen_t.items():
        assert np.array_equal(t.view(U32), seen_t[first].view(U32)), (first, what)
    first = next(iter(seen_b))
    for what, b in seen_b.items():
        assert np.array_equal(b, seen_b[first]), (first, what)
    assert len(seen_t) >= (len(BUILDERS) * len(FRAMES) * (3 if nb else 2)) and len(seen_b) == len(BUILDERS) * len(FRAMES) * len(walks)
    print(name, "rays", rays.n, "hit share %.3f" % float((B.t > 0).mean()), "blocked share %.3f" % float(B.blocked.mean()),
          "closest queries", len(seen_t), "shadow queries", len(seen_b))


def test_empty_scene_answers_planes_only(gpu, renderer):
    scene, objs, rays, rows, B = gpu.get("count0")
    assert not HM.is_bounded(objs).any() and (B.t > 0).any() and (B.t == 0).any()
    renderer.upload(scene)
    got = renderer.trace_rays(rays.o, rays.d)
    hit = got["t"] > 0
    assert np.array_equal(hit, B.t > 0) and (objs["type"][got["object"][hit]] == abi.RTX_PLANE).all()
    assert renderer.bvh2()["root_ref"] == 0xFFFFFFFF and len(renderer.wide_tree()[0]) == 0
